// rrt_kernel.hip -- general path (any max_ray_depth): one lane = one pixel, the reference's
// recursion unrolled (reference: part1_code.cpp:15-187), plus the small utility kernels
// (tile unpack, tonemap) and the C++ launch shims used by rrt_host.cpp.
//
// Work decomposition: persistent grid; each wave pulls 8x8 pixel blocks (one lane = one pixel,
// the whole adaptive sample loop) from a device atomic over the caller's tile list.  BVH
// traversal is stackless over skip pointers (rrt_internal.h DNode), which visits exactly the
// reference's left-then-right recursion order.  The depth <= 1 hot path runs in the
// sample-parallel batch kernel of rrt_sample.hip instead.
#include "rrt_integrator.h"

#include <cstdlib>
#include <type_traits>

namespace rrt {

// What observer_ray found for a camera sample of the observer's build (V_KERR_OBS): the
// energy ratios E_camera / E_static and E_camera / E_infinity, and whether the factors apply at all
// (not under the identity observer or RRT_OBSERVER_NO_BEAMING)
struct ObsFac { double dv, dd; bool on; };

// of: the observer's build only -- the sample's factors, each applied once: the sky x w(D), the disk's
// colour rule at g x D, a surface hit's whole sample x w(D_v)
template <bool DEEP, bool COUNT, int LEAN, int W = 0, class LV = LevelsPriv>
__device__ __forceinline__ spec est_radiance(const KParams& kp, Rng& g, v3 o, v3 d, Counters& cn, LV lv = LV(),
                                             const ObsFac* of = nullptr) {  // :103-123
  Isect is;
  if constexpr (is_obs(LEAN)) {
    // the disk builds' rule below with every choice at run time, and the observer's factors
    ExitRec xr = {V(0.0, 0.0, 0.0), false};
    DiskRecOf<LEAN> dk; dk.rgb = S(0, 0, 0); dk.hit = false;
    if (!trace<false, COUNT, DEEP, LEAN>(kp, o, d, &is, cn, kp.disk.lensed ? &xr : nullptr, &dk)) {
      if (!kp.env.w) return S(0, 0, 0);
      if (kp.disk.lensed && !xr.escaped) return S(0, 0, 0);
      const spec sky = env_dir(kp.env, kp.disk.lensed ? xr.e : d);
      return of->on ? sky * observer_w(of->dd) : sky;
    }
    if (dk.hit) return of->on ? disk_rgb_rt(kp.disk, dk.r, dk.g * of->dd) : dk.rgb;
    const spec e = emission(kp.bsdfs[is.bsdf]);
    spec L = e;
    if (kp.max_ray_depth == 1) L = e + one_bounce<COUNT, LEAN, DEEP>(kp, g, is, cn);
    else if (kp.max_ray_depth >= 2) L = e + at_least_one_bounce<COUNT, general_of(LEAN)>(kp, g, is, cn, lv);
    return of->on ? L * observer_w(of->dv) : L;
  } else if (is_disk(LEAN)) {
    // the disk build: a camera ray that reaches the disk returns its radiance; a miss takes the sky
    // rule in force -- the lensed sky's (the far march runs) or the reference's (it does not)
    ExitRec xr = {V(0.0, 0.0, 0.0), false};
    DiskRec dk = {S(0, 0, 0), false};
    if (!trace<false, COUNT, DEEP, LEAN>(kp, o, d, &is, cn, kp.disk.lensed ? &xr : nullptr, &dk)) {
      if (!kp.env.w) return S(0, 0, 0);
      if (!kp.disk.lensed) return env_dir(kp.env, d);
      return xr.escaped ? env_dir(kp.env, xr.e) : S(0, 0, 0);
    }
    if (dk.hit) return dk.rgb;
  } else if (is_sky(LEAN)) {  // lensed sky: the map along an escaping ray's exit direction; the hole's shadow is black
    ExitRec xr = {V(0.0, 0.0, 0.0), false};
    if (!trace<false, COUNT, DEEP, LEAN>(kp, o, d, &is, cn, &xr))
      return (xr.escaped && kp.env.w) ? env_dir(kp.env, xr.e) : S(0, 0, 0);
  } else if (camera_proven_miss<COUNT, LEAN == V_KERR, LEAN == 0, W>(kp, o, d, cn) ||
             !trace<false, COUNT, DEEP, LEAN>(kp, o, d, &is, cn))  // miss: envLight->sample_dir(r), unbent r
    return (!is_lean(LEAN) && kp.env.w) ? env_dir(kp.env, d) : S(0, 0, 0);
  if (LEAN == V_SW && sw_illum(kp) != 2u) {  // ILLUM 0 / 1 / 3 (:108-122)
    const uint32_t il = sw_illum(kp);
    if (il == 0u)  // normal_shading (pathtracer.h:199-201): Spectrum(n) * .5 + Spectrum(.5, .5, .5)
      return S((float)is.n.x, (float)is.n.y, (float)is.n.z) * (float).5 + S(.5f, .5f, .5f);
    if (il == 1u) return one_bounce<COUNT, LEAN, DEEP>(kp, g, is, cn);
    return at_least_one_bounce<COUNT, LEAN>(kp, g, is, cn, lv);
  }
  spec e = emission(kp.bsdfs[is.bsdf]);
  if (kp.max_ray_depth == 0) return e;
  if (!DEEP || kp.max_ray_depth == 1) return e + one_bounce<COUNT, LEAN, DEEP>(kp, g, is, cn);
  return e + at_least_one_bounce<COUNT, general_of(LEAN)>(kp, g, is, cn, lv);
}

// PathTracer::raytrace_pixel (:125-163): ADAPTIVE 1, THIN_LENS 0 -- or, in the V_SW build, as kp.sw says
template <bool DEEP, bool COUNT, int LEAN, int W = 0, class LV = LevelsPriv>
__device__ __forceinline__ spec raytrace_pixel(const KParams& kp, uint32_t x, uint32_t y, int& count, Rng& g, Counters& cn,
                                               LV lv = LV()) {
  spec ret = S(0, 0, 0);
  int n = 0;  // samples taken (the reference's i after its loop; counted explicitly: the
              // `++i; break;` form was miscompiled in the register-starved bounce build)
  double s1 = 0.0, s2 = 0.0;
  const DCamera& cam = kp.cam;
  // (this loop restates rrt_device.h sample_pos, sensor_point / pixel_ray_dir and adaptive_stop: through
  // the helpers m3 ran 1.1 % slower, outside the parent's spread -- profiles/rules_once_ab.txt)
  for (int i = 0; i < (int)kp.ns_aa; ++i) {
    double sx = (double)x, sy = (double)y;
    if (kp.ns_aa == 1) { sx += 0.5; sy += 0.5; }
    else { double jx, jy; g.grid(jx, jy); sx += jx; sy += jy; }
    double cx = sx / kp.frame_w, cy = sy / kp.frame_h;
    double vx = (1 - cx) * cam.blx + cx * -cam.blx, vy = (1 - cy) * cam.bly + cy * -cam.bly;
    spec s;
    if (LEAN == V_SW && (kp.sw & SW_THIN_LENS)) {
      // Camera::generate_ray_for_thin_lens (camera.cpp:176-184) at the lens sample the grid sampler
      // draws after the jitter (part1_code.cpp:137-139): rndR = its x, rndTheta = its y * 2 * M_PI
      double lx, ly; g.grid(lx, ly);
      const double rnd_theta = ly * 2 * PI_D;
      const double lr = kp.lens_r * sqrt(lx);
      const v3 pl = V(lr * rrt_glibm_cos(rnd_theta), lr * rrt_glibm_sin(rnd_theta), 0);
      const v3 c0 = ld3(cam.c2w0), c1 = ld3(cam.c2w1), c2 = ld3(cam.c2w2);
      const v3 o = ld3(cam.pos) + ((smul(pl.x, c0) + smul(pl.y, c1)) + smul(pl.z, c2));  // pos + c2w * pLens
      const v3 q = V(vx * kp.focal, vy * kp.focal, -1.0 * kp.focal) - pl;                // pinHole * f - pLens
      s = est_radiance<DEEP, COUNT, LEAN, W>(kp, g, o, unit((smul(q.x, c0) + smul(q.y, c1)) + smul(q.z, c2)), cn, lv);
    } else {
      // Camera::generate_ray (part1_code.cpp:182-187)
      v3 w = (smul(vx, ld3(cam.c2w0)) + smul(vy, ld3(cam.c2w1))) + smul(-1.0, ld3(cam.c2w2));
      if constexpr (is_obs(LEAN)) {
        // the moving observer: the generated direction is the camera's rest frame's; the
        // identity observer (a launch constant: a wave-uniform branch) passes it through untouched
        v3 dn = unit(w);
        ObsFac of = {1.0, 1.0, false};
        if (!kp.obs.identity) {
          dn = observer_ray(kp.obs, dn, of.dv, of.dd);
          of.on = !kp.obs.no_beaming;
        }
        s = est_radiance<DEEP, COUNT, LEAN, W>(kp, g, ld3(cam.pos), dn, cn, lv, &of);
      } else {
        s = est_radiance<DEEP, COUNT, LEAN, W>(kp, g, ld3(cam.pos), unit(w), cn, lv);
      }
    }
    ret = ret + s;
    if (LEAN == V_SW && (kp.sw & SW_NO_ADAPTIVE)) { n = i + 1; continue; }  // ADAPTIVE 0
    double il = illum(s);
    s1 += il;
    s2 += il * il;
    n = i + 1;
    // The opt-in builds (lensed sky, disk): n must be the lane's own value.  i is the same in every lane
    // that is still in the loop; in V_KERR_DISK_LIGHT a lane that broke below while others went on
    // reported a later n after the loop -- count came out as ns_aa and rgb divided by it, the draws
    // right (tests/test_gpu_deep_builds.py).  Passing n through a vector register here
    // makes it per-lane; a constant-false condition in every other build.
    if (is_sky(LEAN) || is_disk(LEAN)) asm volatile("" : "+v"(n));
    if ((uint32_t)n % kp.samples_per_batch == 0) {
      double avg = s1 / n, sd = sqrt((s2 - avg * s1) / i);
      if (1.96 * sd / sqrt((double)n) <= (double)kp.max_tolerance * avg) break;
    }
  }
  count = n;
  return ret / (float)n;
}

}  // namespace rrt

// ------------------------------------------------------------------ kernels
// DEEP: max_ray_depth >= 2 (bounce loop); COUNT: per-pixel work counters; LEAN: area lights
// only, no microfacet BSDF, importance-sampled direct light (the BASELINE scenes); WAVES: the
// register budget, as minimum waves per SIMD; LVD: 0, or the depth bound of the bounce levels kept
// in LDS (rrt_integrator.h LevelsLds; frames of max_ray_depth <= LVD).
template <bool DEEP, bool COUNT, int LEAN, int WAVES, int LVD = 0>
__global__ __launch_bounds__(256, WAVES) void rrt_render_kernel(const KParams* __restrict__ kpp) {
  const KParams& kp = *kpp;
  using namespace rrt;
  using LV = std::conditional_t<(LVD > 0), LevelsLds<(LVD > 0 ? LVD : 1)>, LevelsPriv>;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t bpt = kp.blocks_per_tile_side;
  const uint32_t tpix = kp.tile_size * kp.tile_size;
  for (;;) {
    uint32_t blk = 0;
    if (lane == 0) blk = atomicAdd(kp.block_counter, kp.claim_list ? 64u : 1u);
    blk = __shfl(blk, 0);
    // (restates rrt_device.h claim_pixel / block_pixel, in_clip and write_pixel / write_counters, as above)
    uint32_t t, lx, ly;
    bool mine;
    if (kp.claim_list) {  // the pixel proof pass's list: 64 listed pixels per claim, one per lane
      const uint32_t n_list = *kp.claim_count;
      if (blk >= n_list) break;
      const uint32_t e = blk + lane;
      mine = e < n_list;
      const uint32_t ix = mine ? (kp.claim_list[e] & 0x7fffffffu) : 0u;
      t = kp.tile_order[ix / tpix];
      const uint32_t r = claim_r(ix % tpix, kp.tile_size);
      lx = r % kp.tile_size; ly = r / kp.tile_size;
    } else {
      if (blk >= kp.n_blocks) break;
      t = blk / (bpt * bpt);
      const uint32_t b = blk % (bpt * bpt);
      lx = (b % bpt) * 8 + (lane & 7u); ly = (b / bpt) * 8 + (lane >> 3);
      mine = true;
    }
    const uint32_t x = kp.tiles[2 * t] + lx, y = kp.tiles[2 * t + 1] + ly;
    if (mine && lx < kp.tile_size && ly < kp.tile_size && x >= kp.clip_x0 && y >= kp.clip_y0 && x < kp.clip_x1 &&
        y < kp.clip_y1) {
      Rng g; g.key = rrt_pixel_key(kp.seed, x, y); g.ctr = 0;
      Counters cn = {0, 0, 0, 0};
      int cnt;
      LV lv;
      if constexpr (LVD > 0) {
        __shared__ LevelLds<(LVD > 0 ? LVD : 1)> lvs;
        lv = LV{&lvs, threadIdx.x};
      }
      spec s = raytrace_pixel<DEEP, COUNT, LEAN, 16 * DEEP + 8 * COUNT + WAVES>(kp, x, y, cnt, g, cn, lv);
      const size_t k = (size_t)t * tpix + (size_t)ly * kp.tile_size + lx;
      kp.rgb[3 * k] = s.r; kp.rgb[3 * k + 1] = s.g; kp.rgb[3 * k + 2] = s.b;
      kp.count[k] = cnt;
      if (kp.draws) kp.draws[k] = g.ctr;
      if (COUNT && kp.counters) {
        kp.counters[4 * k] = cn.bbox; kp.counters[4 * k + 1] = cn.micro;
        kp.counters[4 * k + 2] = cn.prim; kp.counters[4 * k + 3] = cn.query;
      }
    }
  }
}

__global__ void rrt_unpack_kernel(const uint32_t* tiles, uint32_t n_tiles, uint32_t ts, uint32_t fw, uint32_t fh,
                                  const float* rgb_p, const int32_t* cnt_p, float* rgb, int32_t* cnt) {
  const size_t tpix = (size_t)ts * ts;
  const size_t total = tpix * n_tiles;
  for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < total; k += (size_t)gridDim.x * blockDim.x) {
    const size_t t = k / tpix, r = k % tpix;
    const uint32_t x = tiles[2 * t] + (uint32_t)(r % ts), y = tiles[2 * t + 1] + (uint32_t)(r / ts);
    if (x < fw && y < fh && (r % ts) < ts) {
      const size_t o = (size_t)y * fw + x;
      rgb[3 * o] = rgb_p[3 * k]; rgb[3 * o + 1] = rgb_p[3 * k + 1]; rgb[3 * o + 2] = rgb_p[3 * k + 2];
      cnt[o] = cnt_p[k];
    }
  }
}

// HDRImageBuffer::toColor (image.h:183-198) + ImageBuffer::update_pixel (image.h:53-62)
__global__ void rrt_tonemap_kernel(uint32_t n, const float* rgb, uint32_t* out, float exposure, float inv_gamma) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    float r = powf(rgb[3 * k] * exposure, inv_gamma);
    float g = powf(rgb[3 * k + 1] * exposure, inv_gamma);
    float b = powf(rgb[3 * k + 2] * exposure, inv_gamma);
    // clamp(0.f, 1.f, c) == std::min(std::max(0.f, 1.f), c) == min(1, c) (misc.h:66-69)
    r = (r < 1.f) ? r : 1.f; g = (g < 1.f) ? g : 1.f; b = (b < 1.f) ? b : 1.f;
    uint32_t p = 0;
    p |= ((uint32_t)(b * 255)) << 16;
    p |= ((uint32_t)(g * 255)) << 8;
    p |= ((uint32_t)(r * 255));
    p |= 0xFF000000u;
    out[k] = p;
  }
}

// The device's restatements of the host C library's functions (rrt_glibm.h), evaluated on n
// arguments: rrt_libm_eval checks them bit for bit against the host's libm (tests/test_gpu_glibm.py).
// fn: 0 sin, 1 cos, 2 acos, 3 atan2(a, b), 4 sinf((float)a), 5 cosf((float)a), 6 exp, 7 log, 8 erf,
// 9 atan, 10 tan
__global__ void rrt_libm_kernel(int fn, uint64_t n, const double* a, const double* b, double* out) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const double x = a[k];
    double r;
    switch (fn) {
      case 0: r = rrt_glibm_sin(x); break;
      case 1: r = rrt_glibm_cos(x); break;
      case 2: r = rrt_glibm_acos(x); break;
      case 3: r = rrt_glibm_atan2(x, b[k]); break;
      case 4: r = rrt_glibm_sinf((float)x); break;
      case 5: r = rrt_glibm_cosf((float)x); break;
      case 6: r = rrt_glibm_exp(x); break;
      case 7: r = rrt_glibm_log(x); break;
      case 8: r = rrt_glibm_erf(x); break;
      case 9: r = rrt_glibm_atan(x); break;
      default: r = rrt_glibm_tan(x); break;
    }
    out[k] = r;
  }
}
// EnvironmentLight::sample_dir as the kernels evaluate it (rrt_device.h env_dir) on n directions:
// rrt_env_eval, the checker's handle on the lensed sky's lookups (tests/test_gpu_lensed_sky.py)
__global__ void rrt_env_kernel(const DEnv env, uint64_t n, const double* dirs, float* rgb) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const rrt::spec s = rrt::env_dir(env, rrt::V(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]));
    rgb[3 * k] = s.r; rgb[3 * k + 1] = s.g; rgb[3 * k + 2] = s.b;
  }
}
// The disk's colour as the march evaluates it (rrt_device.h disk_rgb, plain or blackbody) at n radii
// r_m (Boyer-Lindquist r in M; x m: scene units) and redshifts g: rrt_disk_eval, the checker's handle
// on radii and redshifts no camera ray reaches (tests/test_gpu_blackbody.py)
__global__ void rrt_disk_kernel(const DDisk disk, double m, uint64_t n, const double* r_m, const double* g, float* rgb) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const double r = r_m[k] * m;
    const rrt::spec s = disk.blackbody ? rrt::disk_rgb<true>(disk, r, g[k]) : rrt::disk_rgb<false>(disk, r, g[k]);
    rgb[3 * k] = s.r; rgb[3 * k + 1] = s.g; rgb[3 * k + 2] = s.b;
  }
}
// ... of a blackbody disk with the Page-Thorne profile (disk_rgb<true, true>): a kernel of
// its own, so that rrt_disk_kernel stays the code it was
__global__ void rrt_disk_pt_kernel(const DDisk disk, double m, uint64_t n, const double* r_m, const double* g, float* rgb) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const rrt::spec s = rrt::disk_rgb<true, true>(disk, r_m[k] * m, g[k]);
    rgb[3 * k] = s.r; rgb[3 * k + 1] = s.g; rgb[3 * k + 2] = s.b;
  }
}
// The disk light's sampler as disk_direct evaluates it (rrt_device.h disk_sample) on n
// shading points p [n][3] and draws uv [n][2]: rrt_disk_sample, the checker's handle on points and
// draws no frame reaches (tests/test_gpu_disk_light.py).  An invalid sample: pdf 0.
__global__ void rrt_disk_sample_kernel(const DHole hole, const DDisk disk, uint64_t n, const double* p, const double* uv,
                                       double* wi, float* pdf) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    rrt::v3 w;
    float f;
    const bool ok = rrt::disk_sample(hole, disk, rrt::V(p[3 * k], p[3 * k + 1], p[3 * k + 2]), uv[2 * k], uv[2 * k + 1], w, f);
    wi[3 * k] = w.x; wi[3 * k + 1] = w.y; wi[3 * k + 2] = w.z;
    pdf[k] = ok ? f : 0.0f;
  }
}

// The moving observer's rule as the render kernel evaluates it (rrt_device.h observer_ray)
// on n caller directions np [n][3]: rrt_observer_eval, the checker's handle.  The identity observer
// passes the direction through with both ratios 1, as raytrace_pixel does.
__global__ void rrt_observer_kernel(const DObs obs, uint64_t n, const double* np, double* d_eff, double* dv, double* dd) {
  for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    rrt::v3 d = rrt::V(np[3 * k], np[3 * k + 1], np[3 * k + 2]);
    double v = 1.0, w = 1.0;
    if (!obs.identity) d = rrt::observer_ray(obs, d, v, w);
    d_eff[3 * k] = d.x; d_eff[3 * k + 1] = d.y; d_eff[3 * k + 2] = d.z;
    dv[k] = v; dd[k] = w;
  }
}

// ------------------------------------------------------------------ launch shims (C++ linkage)
// Kernel selection: deep / counting variants are built once (1 wave per SIMD budget); the
// depth <= 1 path has general and LEAN builds at 1..4 waves per SIMD (A/B knob `waves`).
// variant = the kernel build (rrt_internal.h V_*), as rrt_host.cpp choose_variant chose it.
hipError_t rrt_launch_render(const KParams& kp, const KParams* d_kp, int deep, int count, int variant, int waves, uint32_t grid,
                             hipStream_t stream) {
#define RRT_LAUNCH(D, C, L, W) hipLaunchKernelGGL((rrt_render_kernel<D, C, L, W>), dim3(grid), dim3(256), 0, stream, d_kp)
  // the bounce levels in LDS (frames of max_ray_depth <= 4; RRT_AB_NO_LEVEL_LDS=1 keeps them private, A/B)
  static const bool no_lv = [] { const char* e = std::getenv("RRT_AB_NO_LEVEL_LDS"); return e && e[0] == '1'; }();
  const bool lv4 = deep && !count && kp.max_ray_depth <= 4u && !no_lv;
  // The lensed sky (one build per metric) and the accretion disk (plain, blackbody DESIGN.md §13, sampled
  // as a light §14, Page-Thorne §15: builds of their own): bounce-capable, no counters, 2 waves/SIMD
  // (cfg3's framing 141.8 -> 117.4 ms against 1; the cfg5 crop the same, profiles/README.md)
  switch (variant) {
#define RRT_SKY_DISK(V) case rrt::V: RRT_LAUNCH(true, false, rrt::V, 2); return hipGetLastError();
    RRT_SKY_DISK(V_SKY) RRT_SKY_DISK(V_KERR_SKY)
    RRT_SKY_DISK(V_KERR_DISK) RRT_SKY_DISK(V_KERR_DISK_BB)
    RRT_SKY_DISK(V_KERR_DISK_LIGHT) RRT_SKY_DISK(V_KERR_DISK_BB_LIGHT)
    RRT_SKY_DISK(V_KERR_DISK_PT) RRT_SKY_DISK(V_KERR_DISK_PT_LIGHT)
    RRT_SKY_DISK(V_KERR_OBS)  // the moving observer's build
#undef RRT_SKY_DISK
    default: break;
  }
  if (variant == rrt::V_SW) {  // the reference's switches as run-time flags: one bounce-capable build
    if (count) RRT_LAUNCH(true, true, rrt::V_SW, 1); else RRT_LAUNCH(true, false, rrt::V_SW, 1);
  } else if (variant == rrt::V_KERR) {  // the Kerr builds (general integrator)
    if (deep) {
      if (count) RRT_LAUNCH(true, true, rrt::V_KERR, 1); else RRT_LAUNCH(true, false, rrt::V_KERR, 1);
    } else if (count) {
      RRT_LAUNCH(false, true, rrt::V_KERR, 1);
    } else {
      RRT_LAUNCH(false, false, rrt::V_KERR, 2);
    }
  } else if (deep) {
    if (count) {
      RRT_LAUNCH(true, true, false, 1);
    } else {
      if (lv4 && (waves == 3 || waves <= 0 || waves > 4)) {
        hipLaunchKernelGGL((rrt_render_kernel<true, false, false, 3, 4>), dim3(grid), dim3(256), 0, stream, d_kp);
        return hipGetLastError();
      }
      switch (waves) {  // register budget (A/B): the bounce build spills below 1 wave/SIMD's 256 VGPRs
        case 2: RRT_LAUNCH(true, false, false, 2); break;
        case 3: RRT_LAUNCH(true, false, false, 3); break;
        case 4: RRT_LAUNCH(true, false, false, 4); break;
        case 1: RRT_LAUNCH(true, false, false, 1); break;
        default: RRT_LAUNCH(true, false, false, 3); break;
      }
    }
  } else if (count) {
    RRT_LAUNCH(false, true, false, 1);
  } else if (variant == rrt::V_LEAN) {  // V_LEAN_POINT runs the general build here
    switch (waves) {
      case 1: RRT_LAUNCH(false, false, true, 1); break;
      case 3: RRT_LAUNCH(false, false, true, 3); break;
      case 4: RRT_LAUNCH(false, false, true, 4); break;
      default: RRT_LAUNCH(false, false, true, 2); break;
    }
  } else {
    if (waves == 1) RRT_LAUNCH(false, false, false, 1); else RRT_LAUNCH(false, false, false, 2);
  }
#undef RRT_LAUNCH
  return hipGetLastError();
}
hipError_t rrt_launch_unpack(const uint32_t* tiles, uint32_t n_tiles, uint32_t ts, uint32_t fw, uint32_t fh,
                             const float* rgb_p, const int32_t* cnt_p, float* rgb, int32_t* cnt, hipStream_t stream) {
  size_t total = (size_t)ts * ts * n_tiles;
  uint32_t grid = (uint32_t)((total + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rrt_unpack_kernel, dim3(grid), dim3(256), 0, stream, tiles, n_tiles, ts, fw, fh, rgb_p, cnt_p,
                     rgb, cnt);
  return hipGetLastError();
}
hipError_t rrt_launch_libm(int fn, uint64_t n, const double* a, const double* b, double* out, hipStream_t stream) {
  uint64_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rrt_libm_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, fn, n, a, b, out);
  return hipGetLastError();
}
hipError_t rrt_launch_env(const DEnv& env, uint64_t n, const double* dirs, float* rgb, hipStream_t stream) {
  uint64_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rrt_env_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, env, n, dirs, rgb);
  return hipGetLastError();
}
hipError_t rrt_launch_disk(const DDisk& disk, double m, uint64_t n, const double* r_m, const double* g, float* rgb,
                           hipStream_t stream) {
  uint64_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  if (grid == 0) grid = 1;
  if (disk.blackbody && disk.profile == RRT_DISK_PROFILE_PAGE_THORNE)
    hipLaunchKernelGGL(rrt_disk_pt_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, disk, m, n, r_m, g, rgb);
  else
    hipLaunchKernelGGL(rrt_disk_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, disk, m, n, r_m, g, rgb);
  return hipGetLastError();
}
hipError_t rrt_launch_disk_sample(const DHole& hole, const DDisk& disk, uint64_t n, const double* p, const double* uv,
                                  double* wi, float* pdf, hipStream_t stream) {
  uint64_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rrt_disk_sample_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, hole, disk, n, p, uv, wi, pdf);
  return hipGetLastError();
}
hipError_t rrt_launch_observer(const DObs& obs, uint64_t n, const double* np, double* d_eff, double* dv, double* dd,
                               hipStream_t stream) {
  uint64_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rrt_observer_kernel, dim3((uint32_t)grid), dim3(256), 0, stream, obs, n, np, d_eff, dv, dd);
  return hipGetLastError();
}
hipError_t rrt_launch_tonemap(uint32_t n, const float* rgb, uint32_t* out, float exposure, float inv_gamma,
                              hipStream_t stream) {
  uint32_t grid = (n + 255) / 256;
  if (grid > 4096) grid = 4096;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(rrt_tonemap_kernel, dim3(grid), dim3(256), 0, stream, n, rgb, out, exposure, inv_gamma);
  return hipGetLastError();
}
