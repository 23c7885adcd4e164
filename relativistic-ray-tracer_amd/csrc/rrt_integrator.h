// rrt_integrator.h -- the reference's integrator (part1_code.cpp:15-101): direct lighting by
// importance or hemisphere sampling and at_least_one_bounce_radiance's recursion as a loop, over
// the geodesic-marched query.  Shared by the per-pixel-loop kernel (rrt_kernel.hip) and the
// per-sample refill kernel (rrt_sample.hip) for max_ray_depth >= 2.
#pragma once
#include "rrt_device.h"

#include <type_traits>

namespace rrt {

// ------------------------------------------------------------------ integrator (part1_code.cpp)
// `trace` = the geodesic-marched BVH query; DEEP (bounce) builds and depth <= 1 builds share it.
// The lensed-sky builds (V_SKY, V_KERR_SKY) run the exit-mode march for every query; xr: where the
// ray went if it hit nothing (they only).
// The disk builds (V_KERR_DISK; V_KERR_DISK_BB, §13: the blackbody colour) run the
// exit-mode march with the disk test; its far march runs only where xr is given (the lensed sky's rule
// in force).  dk: a hit that is the disk.  Their _LIGHT builds (§14) trace as their parents; the _PT
// builds (§15) as V_KERR_DISK_BB with the Page-Thorne profile.
template <bool ANY, bool COUNT, bool DEEP, int LEAN>
__device__ __forceinline__ bool trace(const KParams& kp, v3 o, v3 d, Isect* is, Counters& cn, ExitRec* xr = nullptr,
                                      DiskRec* dk = nullptr) {
  return query<ANY, COUNT, is_kerr_build(LEAN), is_lean(LEAN), is_sky(LEAN) || is_disk(LEAN), is_disk(LEAN),
               is_disk_bb(LEAN), is_disk_pt(LEAN), false, is_obs(LEAN)>(kp, o, d, is, cn, false, nullptr, xr, dk);
}
// the disk record of a build's marches: the observer's build (RT march) takes the crossing's r and g too
template <int LEAN>
using DiskRecOf = std::conditional_t<is_obs(LEAN), DiskRecRT, DiskRec>;
// the emission a ray picks up at its hit: the hit primitive's BSDF's, or the disk's radiance
__device__ __forceinline__ spec hit_emission(const KParams& kp, const Isect& is, const DiskRec& dk) {
  return dk.hit ? dk.rgb : emission(kp.bsdfs[is.bsdf]);
}

// LEAN: area/point lights only, no microfacet BSDF.  The shading frame is rebuilt per light sample
// (same values: make_coord_space is a pure function of the normal) instead of being kept live
// across the shadow query, which keeps 12 VGPRs out of the traversal loop.
template <bool COUNT, int LEAN, bool DEEP>
__device__ spec direct_importance(const KParams& kp, Rng& g, const Isect& is, Counters& cn) {  // :33-57
  const DBsdf b = kp.bsdfs[is.bsdf];
  spec L = S(0, 0, 0);
  int total = 0;
  for (uint32_t li = 0; li < kp.n_lights; ++li) {
    const DLight& l = kp.lights[li];
    int num = l.is_delta ? 1 : (int)kp.ns_area_light;
    total += num;
    for (int i = 0; i < num; ++i) {
      v3 wi_world; float dist, pdf;
      spec sample = light_sample_L<LEAN>(kp.env, l, g, is.hit_p, wi_world, dist, pdf,
                                         LEAN == V_SW && (kp.sw & SW_ENV_HEMI));
      const Frame f = coord_space(is.n);
      v3 w_in = to_local(f, wi_world);
      if (w_in.z < 0) continue;
      if ((is_sky(LEAN) || (is_disk(LEAN) && kp.disk.lensed)) && l.type == 5u) {
        // lensed sky: the environment light's sample counts iff its shadow ray escapes, with the
        // map's radiance along the exit direction; wi, pdf, the BSDF term and the draws as they are
        ExitRec xr = {V(0.0, 0.0, 0.0), false};
        if (trace<true, COUNT, DEEP, LEAN>(kp, is.hit_p + smul(EPS_D, wi_world), wi_world, nullptr, cn, &xr) || !xr.escaped)
          continue;
        L = L + ((env_dir(kp.env, xr.e) * bsdf_f<LEAN>(b, to_local(f, is.w_out), w_in)) * (float)w_in.z) / pdf;
        continue;
      }
      spec contrib = ((sample * bsdf_f<LEAN>(b, to_local(f, is.w_out), w_in)) * (float)w_in.z) / pdf;
      if (!trace<true, COUNT, DEEP, LEAN>(kp, is.hit_p + smul(EPS_D, wi_world), wi_world, nullptr, cn)) L = L + contrib;
    }
  }
  return L / (float)total;
}

template <bool COUNT, int LEAN, bool DEEP>
__device__ spec direct_hemisphere(const KParams& kp, Rng& g, const Isect& is, Counters& cn) {  // :15-31
  Frame f = coord_space(is.n);
  v3 w_out = to_local(f, is.w_out);
  const DBsdf b = kp.bsdfs[is.bsdf];
  int num = (int)(kp.n_lights * kp.ns_area_light);
  spec L = S(0, 0, 0);
  for (int i = 0; i < num; ++i) {
    v3 w_in = hemisphere_sample(g);
    v3 wi_world = to_world(f, w_in);
    Isect is2;
    if (is_disk(LEAN)) {  // the emitter term takes the disk's radiance where the ray ends on the disk
      DiskRecOf<LEAN> dk; dk.rgb = S(0, 0, 0); dk.hit = false;
      if (trace<false, COUNT, DEEP, LEAN>(kp, is.hit_p + smul(EPS_D, wi_world), wi_world, &is2, cn, nullptr, &dk))
        L = L + (hit_emission(kp, is2, dk) * bsdf_f(b, w_out, w_in)) * (float)w_in.z;
      continue;
    }
    if (trace<false, COUNT, DEEP, LEAN>(kp, is.hit_p + smul(EPS_D, wi_world), wi_world, &is2, cn))
      L = L + (emission(kp.bsdfs[is2.bsdf]) * bsdf_f(b, w_out, w_in)) * (float)w_in.z;
  }
  return ((L * 2.0f) * (float)PI_D) / (float)num;
}

// The disk importance-sampled as a light (RRT_DISK_LIGHT; the _LIGHT disk builds):
// ns_area_light samples of the annulus's flat image (disk_sample; two draws each, as an area light's),
// each evaluated by the closest-hit march along the bent ray: the disk's radiance where that ray
// really meets it, nothing for a primitive in front, a capture or an escape.  Drawn after every listed
// light and normalised by its own sample count, so direct_importance's term and draws stay as they are.
template <bool COUNT, int LEAN, bool DEEP>
__device__ __forceinline__ spec disk_direct(const KParams& kp, Rng& g, const Isect& is, Counters& cn) {
  const DBsdf b = kp.bsdfs[is.bsdf];
  spec L = S(0, 0, 0);
  const int num = (int)kp.ns_area_light;
  if (num == 0) return L;
  for (int i = 0; i < num; ++i) {
    double u, v;
    g.grid(u, v);
    v3 wi_world; float pdf;
    if (!disk_sample(kp.hole, kp.disk, is.hit_p, u, v, wi_world, pdf)) continue;
    const Frame f = coord_space(is.n);
    v3 w_in = to_local(f, wi_world);
    if (w_in.z < 0) continue;
    Isect is2;
    DiskRecOf<LEAN> dk; dk.rgb = S(0, 0, 0); dk.hit = false;
    if (!trace<false, COUNT, DEEP, LEAN>(kp, is.hit_p + smul(EPS_D, wi_world), wi_world, &is2, cn, nullptr, &dk) || !dk.hit)
      continue;
    L = L + ((dk.rgb * bsdf_f<LEAN>(b, to_local(f, is.w_out), w_in)) * (float)w_in.z) / pdf;
  }
  return L / (float)num;
}

template <bool COUNT, int LEAN, bool DEEP>
__device__ __forceinline__ spec one_bounce(const KParams& kp, Rng& g, const Isect& is, Counters& cn) {
  if (is_lean(LEAN)) return direct_importance<COUNT, LEAN, DEEP>(kp, g, is, cn);
  if (is_disk_light(LEAN) && kp.disk.light && !kp.direct_hemisphere) {
    const spec Ll = direct_importance<COUNT, LEAN, DEEP>(kp, g, is, cn);  // the listed lights first: their draws
    return Ll + disk_direct<COUNT, LEAN, DEEP>(kp, g, is, cn);
  }
  return kp.direct_hemisphere ? direct_hemisphere<COUNT, general_of(LEAN), DEEP>(kp, g, is, cn)
                              : direct_importance<COUNT, general_of(LEAN), DEEP>(kp, g, is, cn);
}

// The per-level terms of at_least_one_bounce (the recursion's pending values): the level's direct
// light Ld, its flags (child: the bounce ray hit, so the level folds the child's radiance in; dl: the
// BSDF is a delta), and for a child the BSDF sample, |cos|, pdf and the hit's emission.
// LevelsPriv: private arrays, any depth <= RRT_MAX_DEPTH (they live in scratch: dynamic indices).
struct LevelsPriv {
  static constexpr int D = RRT_MAX_DEPTH;
  spec Ld[D], smp[D], cem[D];
  float cs[D], pd[D];
  bool child[D], dl[D];
  __device__ __forceinline__ void level(int k, spec ld, bool d) { Ld[k] = ld; child[k] = false; dl[k] = d; }
  __device__ __forceinline__ void bounce(int k, spec sm, float c, float p, spec em) {
    child[k] = true; smp[k] = sm; cs[k] = c; pd[k] = p; cem[k] = em;
  }
  __device__ __forceinline__ spec fold(int k) const {
    spec L = S(0, 0, 0);
    for (int j = k; j >= 0; --j) {
      spec Lj = Ld[j];
      if (child[j]) {
        spec Lc = L;
        if (dl[j]) Lc = Lc + cem[j];
        Lj = Lj + (((Lc * smp[j]) * cs[j]) / pd[j]) / (float)0.7;
      }
      L = Lj;
    }
    return L;
  }
};
// LevelsLds: the same terms in LDS, one column per thread of a 256-thread block, for frames of
// max_ray_depth <= D (the loop then never reaches RRT_MAX_DEPTH's cap): the bounce kernel's levels
// left scratch, whose writes were most of its HBM traffic (bounce paths).
template <int D_>
struct LevelLds {
  float v[11][D_][256];  // Ld rgb, smp rgb, cem rgb, cs, pd
  uint8_t fl[D_][256];   // 1: child, 2: dl
};
template <int D_>
struct LevelsLds {
  static constexpr int D = D_;
  LevelLds<D_>* p;
  uint32_t t;
  __device__ __forceinline__ void level(int k, spec ld, bool d) {
    p->v[0][k][t] = ld.r; p->v[1][k][t] = ld.g; p->v[2][k][t] = ld.b;
    p->fl[k][t] = d ? 2 : 0;
  }
  __device__ __forceinline__ void bounce(int k, spec sm, float c, float pp, spec em) {
    p->v[3][k][t] = sm.r; p->v[4][k][t] = sm.g; p->v[5][k][t] = sm.b;
    p->v[6][k][t] = em.r; p->v[7][k][t] = em.g; p->v[8][k][t] = em.b;
    p->v[9][k][t] = c; p->v[10][k][t] = pp;
    p->fl[k][t] |= 1;
  }
  __device__ __forceinline__ spec fold(int k) const {
    spec L = S(0, 0, 0);
    for (int j = k; j >= 0; --j) {
      spec Lj = S(p->v[0][j][t], p->v[1][j][t], p->v[2][j][t]);
      const uint8_t f = p->fl[j][t];
      if (f & 1) {
        spec Lc = L;
        if (f & 2) Lc = Lc + S(p->v[6][j][t], p->v[7][j][t], p->v[8][j][t]);
        Lj = Lj + (((Lc * S(p->v[3][j][t], p->v[4][j][t], p->v[5][j][t])) * p->v[9][j][t]) / p->v[10][j][t]) / (float)0.7;
      }
      L = Lj;
    }
    return L;
  }
};

// at_least_one_bounce_radiance (:69-101) unrolled into a loop: the recursion is walked down
// storing each level's terms, then folded back up in the reference's evaluation order.
template <bool COUNT, int LEAN, class LV = LevelsPriv>
__device__ __forceinline__ spec at_least_one_bounce(const KParams& kp, Rng& g, Isect cur, Counters& cn, LV lv = LV()) {
  uint32_t depth = kp.max_ray_depth;
  int k = 0;
  for (;; ++k) {
    Frame f = coord_space(cur.n);
    v3 w_out = to_local(f, cur.w_out);
    const DBsdf b = kp.bsdfs[cur.bsdf];
    spec L_out = S(0, 0, 0);
    if (!is_delta(b)) L_out = L_out + one_bounce<COUNT, general_of(LEAN), true>(kp, g, cur, cn);
    if (LEAN == V_SW && sw_illum(kp) == 3u && depth == kp.max_ray_depth) L_out = S(0, 0, 0);  // ILLUM 3 (:78-81)
    lv.level(k, L_out, is_delta(b));
    if (depth == kp.max_ray_depth || (depth > 1 && g.coin(0.7))) {
      v3 w_in; float pdf;
      spec sample = bsdf_sample_f(b, g, w_out, w_in, pdf, LEAN == V_SW && (kp.sw & SW_MF_HEMI));
      if (pdf == 0.0f) break;
      v3 wi_world = to_world(f, w_in);
      Isect is2;
      if (is_disk(LEAN)) {  // a bounce ray that ends on the disk ends the path there
        DiskRecOf<LEAN> dk; dk.rgb = S(0, 0, 0); dk.hit = false;
        if (trace<false, COUNT, true, LEAN>(kp, cur.hit_p + smul(EPS_D, wi_world), wi_world, &is2, cn, nullptr, &dk) &&
            k + 1 < LV::D) {
          lv.bounce(k, sample, (float)fabs(w_in.z), pdf, hit_emission(kp, is2, dk));
          if (dk.hit) break;  // the child level adds nothing: the disk reflects nothing
          cur = is2;
          depth -= 1;
          continue;
        }
        break;
      }
      if (trace<false, COUNT, true, LEAN>(kp, cur.hit_p + smul(EPS_D, wi_world), wi_world, &is2, cn) && k + 1 < LV::D) {
        lv.bounce(k, sample, (float)fabs(w_in.z), pdf, emission(kp.bsdfs[is2.bsdf]));
        cur = is2;
        depth -= 1;
        continue;
      }
    }
    break;
  }
  return lv.fold(k);
}

}  // namespace rrt
