// rrt_query.hip -- batched geodesic ray queries (rrt_trace_rays / rrt_trace_camera, include/rrt.h):
// BVHAccel::intersect (bvh.cpp:103-113) for caller-given rays or the camera's pixel-centre rays,
// one rrt_hit record per ray instead of a pixel.  Every ray is marched exactly (no proofs); the
// walks take query's result-neutral accelerations (empty-space grid, search tree).
//
// Two decompositions, bit-identical records:
//   * lane per ray (both metrics): block b takes rays [256 b, 256 b + 256), one lane each, the
//     render kernels' query() / kerr_march() with the out-record (rrt_device.h QRec);
//   * wave per ray (Schwarzschild): a ray's micro-ray chain does not depend on any BVH result
//     (bvh.cpp:105-110, blackhole.cpp:17-40), so the wave produces 64 segments of the chain first
//     -- every lane steps the same chain, lane l keeps segment 64 r + l -- and then each lane walks
//     its own segment.  Every segment's closest hit starts from max_t = its own length whatever
//     came before (bvh.cpp:104-110), and the reference returns at the first segment with a capture
//     or a hit, so the lowest flagged lane holds the reference's answer.  No LDS, no barrier, no
//     traffic between waves.
// No claim counter, no spin, no wait on another block or kernel: the grid is sized from n.
#include "rrt_device.h"

namespace rrt {

// ray i of the launch: the caller's (three 16-byte loads of the 48-byte rrt_ray), or pixel i's
// centre ray as raytrace_pixel generates it with ns_aa == 1 (part1_code.cpp:132-141, 182-187)
template <bool CAM>
__device__ __forceinline__ void load_ray(const KParams& kp, const TraceArgs& a, uint32_t i, v3& o, v3& d) {
  if (CAM) {
    const uint32_t x = a.x0 + i % a.w, y = a.y0 + i / a.w;
    o = ld3(kp.cam.pos);
    d = pixel_ray_dir(kp, (double)x + 0.5, (double)y + 0.5);
  } else {
    const double2* p = reinterpret_cast<const double2*>(a.rays) + 3 * (size_t)i;
    const double2 q0 = p[0], q1 = p[1], q2 = p[2];
    o = V(q0.x, q0.y, q1.x);
    d = V(q1.y, q2.x, q2.y);
  }
}

// the 96-byte rrt_hit of ray i as six 16-byte stores; full: a closest-hit record (is, qr.slot, qr.t),
// else every hit field is 0 / -1
__device__ __forceinline__ void store_hit(const TraceArgs& a, uint32_t i, uint32_t status, uint32_t steps, bool full,
                                          const Isect& is, const QRec& qr) {
  double2* h = reinterpret_cast<double2*>(a.hits) + 6 * (size_t)i;
  uint4 tail;
  tail.x = status; tail.y = 0xffffffffu; tail.z = 0xffffffffu; tail.w = steps;
  if (full) {
    h[0] = make_double2(is.hit_p.x, is.hit_p.y);
    h[1] = make_double2(is.hit_p.z, is.n.x);
    h[2] = make_double2(is.n.y, is.n.z);
    h[3] = make_double2(is.w_out.x, is.w_out.y);
    h[4] = make_double2(is.w_out.z, qr.t);
    tail.y = a.slot_prim[qr.slot];
    tail.z = (uint32_t)is.bsdf;
  } else {
    const double2 z = make_double2(0.0, 0.0);
    h[0] = z; h[1] = z; h[2] = z; h[3] = z; h[4] = z;
  }
  *reinterpret_cast<uint4*>(h + 5) = tail;
}

}  // namespace rrt

// KERR: the Kerr march; ANY: shadow query (RRT_TRACE_ANY_HIT); CAM: camera rays
template <bool KERR, bool ANY, bool CAM>
__global__ __launch_bounds__(256) void rrt_trace_lane_kernel(const KParams* __restrict__ kpp, const TraceArgs a) {
  using namespace rrt;
  const KParams& kp = *kpp;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  v3 o, d;
  load_ray<CAM>(kp, a, i, o, d);
  Isect is;
  QRec qr = {-1, 0.0, 0u, false};
  Counters cn = {};
  const bool hit = KERR ? kerr_march<ANY, false>(kp, o, d, &is, cn, &qr)
                        : query<ANY, false, false, true>(kp, o, d, &is, cn, false, &qr);
  store_hit(a, i, hit ? RRT_RAY_HIT : qr.captured ? RRT_RAY_CAPTURED : RRT_RAY_MISS, qr.steps, hit && !ANY, is, qr);
}

// Schwarzschild; block b takes rays [4 b, 4 b + 4), one wave each
template <bool ANY, bool CAM>
__global__ __launch_bounds__(256) void rrt_trace_wave_kernel(const KParams* __restrict__ kpp, const TraceArgs a) {
  using namespace rrt;
  const KParams& kp = *kpp;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= a.n) return;  // the whole wave
  v3 o, d;
  load_ray<CAM>(kp, a, i, o, d);
  double max_t = 0.0;
  v3 e = o + vmul(d, max_t);  // micro = Ray(o, d, max_t = 0), bvh.cpp:104
  Isect is;
  QRec qr = {-1, 0.0, 0u, false};
  Counters cn = {};
  const int steps = kp.hole.steps;
  for (int base = 0; base < steps; base += 64) {
    // 1. the round's stretch of the chain, the same values in every lane (query()'s operations in
    // query()'s order); lane l keeps segment base + l; the chain stops at the first capture
    const int n_round = steps - base < 64 ? steps - base : 64;
    v3 so = o, sd = d, se = e;
    double smt = max_t;
    int cap = -1;
    for (int l = 0; l < n_round; ++l) {
      v3 rel;
      double rel2;
      next_micro_at(kp.hole, e, o, d, max_t, rel, rel2);
      // wave-uniform by construction: taken from the first lane, so the branch is a scalar one
      const bool c = __builtin_amdgcn_readfirstlane((int)sphere_t_rel(rel, rel2, kp.hole.r2, d, max_t)) != 0;
      e = o + vmul(d, max_t);
      if (lane == l) { so = o; sd = d; smt = max_t; se = e; }
      if (c) { cap = l; break; }
    }
    // 2. each lane below the capture walks its own segment: its full closest hit (or any hit)
    const int n_seg = cap >= 0 ? cap : n_round;
    bool hit = false;
    if (lane < n_seg) hit = segment_query<ANY, false, true>(kp, so, sd, smt, se, &is, cn, false, &qr);
    // 3. the lowest flagged segment is where the reference's march returns
    const bool captured = lane == cap;
    const uint64_t flagged = __ballot(hit || captured);
    if (flagged) {
      if (lane == __ffsll((unsigned long long)flagged) - 1)
        store_hit(a, i, captured ? RRT_RAY_CAPTURED : RRT_RAY_HIT, (uint32_t)(base + lane) + 1u, hit && !ANY, is, qr);
      return;
    }
    // 4. none: the next round continues from the chain's state (o, d, max_t, e)
  }
  if (lane == 0) store_hit(a, i, RRT_RAY_MISS, (uint32_t)steps, false, is, qr);
}

// ------------------------------------------------------------------ exit mode (RRT_TRACE_EXIT)
// Builds of their own, so the kernels above stay as they are.  DESIGN.md §11.
namespace rrt {
// the record of a march that ended at its escape row (or, Kerr, in the far march): ESCAPED with
// w_out = -e, or MISS; every other hit field 0 / -1
__device__ __forceinline__ void store_exit(const TraceArgs& a, uint32_t i, uint32_t steps, const ExitRec& xr) {
  double2* h = reinterpret_cast<double2*>(a.hits) + 6 * (size_t)i;
  const double2 z = make_double2(0.0, 0.0);
  h[0] = z; h[1] = z; h[2] = z;
  h[3] = xr.escaped ? make_double2(-xr.e.x, -xr.e.y) : z;
  h[4] = xr.escaped ? make_double2(-xr.e.z, 0.0) : z;
  uint4 tail;
  tail.x = xr.escaped ? RRT_RAY_ESCAPED : RRT_RAY_MISS; tail.y = 0xffffffffu; tail.z = 0xffffffffu; tail.w = steps;
  *reinterpret_cast<uint4*>(h + 5) = tail;
}
}  // namespace rrt

// rrt_trace_lane_kernel with the exit-mode march
template <bool KERR, bool ANY, bool CAM>
__global__ __launch_bounds__(256) void rrt_trace_exit_lane_kernel(const KParams* __restrict__ kpp, const TraceArgs a) {
  using namespace rrt;
  const KParams& kp = *kpp;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  v3 o, d;
  load_ray<CAM>(kp, a, i, o, d);
  Isect is;
  QRec qr = {-1, 0.0, 0u, false};
  ExitRec xr = {V(0.0, 0.0, 0.0), false};
  Counters cn = {};
  const bool hit = query<ANY, false, KERR, !KERR, true>(kp, o, d, &is, cn, false, &qr, &xr);
  if (hit || qr.captured) store_hit(a, i, hit ? RRT_RAY_HIT : RRT_RAY_CAPTURED, qr.steps, hit && !ANY, is, qr);
  else store_exit(a, i, qr.steps, xr);
}

// rrt_trace_wave_kernel in exit mode: the escape row is a property of the chain alone, so it is
// found while the chain is generated, wave-uniform; the chain stops there, and lanes at or beyond it
// walk nothing
template <bool ANY, bool CAM>
__global__ __launch_bounds__(256) void rrt_trace_exit_wave_kernel(const KParams* __restrict__ kpp, const TraceArgs a) {
  using namespace rrt;
  const KParams& kp = *kpp;
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= a.n) return;  // the whole wave
  v3 o, d;
  load_ray<CAM>(kp, a, i, o, d);
  double max_t = 0.0;
  v3 e = o + vmul(d, max_t);
  Isect is;
  QRec qr = {-1, 0.0, 0u, false};
  ExitRec xr = {V(0.0, 0.0, 0.0), false};
  Counters cn = {};
  const int steps = kp.hole.steps;
  for (int base = 0; base < steps; base += 64) {
    const int n_round = steps - base < 64 ? steps - base : 64;
    v3 so = o, sd = d, se = e;
    double smt = max_t;
    int cap = -1, esc = -1;
    for (int l = 0; l < n_round; ++l) {
      v3 rel;
      double rel2;
      MicroOut mo;
      next_micro_at(kp.hole, e, o, d, max_t, rel, rel2, &mo);
      // wave-uniform by construction, as the capture flag below: scalar branches
      if (__builtin_amdgcn_readfirstlane((int)!(mo.v > 0.0)) != 0) {
        esc = l;
        exit_dir(mo, xr);
        break;
      }
      const bool c = __builtin_amdgcn_readfirstlane((int)sphere_t_rel(rel, rel2, kp.hole.r2, d, max_t)) != 0;
      e = o + vmul(d, max_t);
      if (lane == l) { so = o; sd = d; smt = max_t; se = e; }
      if (c) { cap = l; break; }
    }
    const int n_seg = cap >= 0 ? cap : esc >= 0 ? esc : n_round;
    bool hit = false;
    if (lane < n_seg) hit = segment_query<ANY, false, true>(kp, so, sd, smt, se, &is, cn, false, &qr);
    const bool captured = lane == cap;
    const uint64_t flagged = __ballot(hit || captured);
    if (flagged) {
      if (lane == __ffsll((unsigned long long)flagged) - 1)
        store_hit(a, i, captured ? RRT_RAY_CAPTURED : RRT_RAY_HIT, (uint32_t)(base + lane) + 1u, hit && !ANY, is, qr);
      return;
    }
    if (esc >= 0) {  // no hit before the escape row
      if (lane == 0) store_exit(a, i, (uint32_t)(base + esc) + 1u, xr);
      return;
    }
  }
  if (lane == 0) store_hit(a, i, RRT_RAY_MISS, (uint32_t)steps, false, is, qr);
}

// ------------------------------------------------------------------ accretion disk (rrt_set_disk)
// Builds of their own again: the Kerr lane-per-ray kernel whose march tests the disk,
// with (EXIT) and without the exit-mode far march.  A ray that ended on the disk: RRT_RAY_DISK, the
// record a closest hit's (hit_p, n = +-ez g, w_out, t) with prim = bsdf = -1; any-hit: status and steps.
template <bool EXIT, bool ANY, bool CAM>
__global__ __launch_bounds__(256) void rrt_trace_disk_lane_kernel(const KParams* __restrict__ kpp, const TraceArgs a) {
  using namespace rrt;
  const KParams& kp = *kpp;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  v3 o, d;
  load_ray<CAM>(kp, a, i, o, d);
  Isect is;
  QRec qr = {-1, 0.0, 0u, false};
  ExitRec xr = {V(0.0, 0.0, 0.0), false};
  DiskRec dk = {S(0, 0, 0), false};
  Counters cn = {};
  const bool hit = kerr_march<ANY, false, EXIT, true>(kp, o, d, &is, cn, &qr, &xr, &dk);
  if (hit && dk.hit) {
    double2* h = reinterpret_cast<double2*>(a.hits) + 6 * (size_t)i;
    const double2 z = make_double2(0.0, 0.0);
    if (ANY) {
      h[0] = z; h[1] = z; h[2] = z; h[3] = z; h[4] = z;
    } else {
      h[0] = make_double2(is.hit_p.x, is.hit_p.y);
      h[1] = make_double2(is.hit_p.z, is.n.x);
      h[2] = make_double2(is.n.y, is.n.z);
      h[3] = make_double2(is.w_out.x, is.w_out.y);
      h[4] = make_double2(is.w_out.z, qr.t);
    }
    uint4 tail;
    tail.x = RRT_RAY_DISK; tail.y = 0xffffffffu; tail.z = 0xffffffffu; tail.w = qr.steps;
    *reinterpret_cast<uint4*>(h + 5) = tail;
  } else if (hit || qr.captured || !EXIT) {
    store_hit(a, i, hit ? RRT_RAY_HIT : qr.captured ? RRT_RAY_CAPTURED : RRT_RAY_MISS, qr.steps, hit && !ANY, is, qr);
  } else {
    store_exit(a, i, qr.steps, xr);
  }
}

// ------------------------------------------------------------------ moving observer (rrt_set_observer)
// A build of its own once more: the camera rays of rrt_trace_camera with an observer set,
// each passed through observer_ray before the march.  The march is rrt_trace_disk_lane_kernel's, the disk
// tested where kp.disk.on says so, and so is the record: pure geometry, what rrt_trace_rays returns for
// (cam.pos, d_eff).
template <bool EXIT, bool ANY>
__global__ __launch_bounds__(256) void rrt_trace_obs_lane_kernel(const KParams* __restrict__ kpp, const TraceArgs a) {
  using namespace rrt;
  const KParams& kp = *kpp;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n) return;
  v3 o, d;
  load_ray<true>(kp, a, i, o, d);
  if (!kp.obs.identity) {
    double dv, dd;
    d = observer_ray(kp.obs, d, dv, dd);
  }
  Isect is;
  QRec qr = {-1, 0.0, 0u, false};
  ExitRec xr = {V(0.0, 0.0, 0.0), false};
  DiskRec dk = {S(0, 0, 0), false};
  Counters cn = {};
  const bool hit = kerr_march<ANY, false, EXIT, true>(kp, o, d, &is, cn, &qr, &xr, &dk);
  if (hit && dk.hit) {
    double2* h = reinterpret_cast<double2*>(a.hits) + 6 * (size_t)i;
    const double2 z = make_double2(0.0, 0.0);
    if (ANY) {
      h[0] = z; h[1] = z; h[2] = z; h[3] = z; h[4] = z;
    } else {
      h[0] = make_double2(is.hit_p.x, is.hit_p.y);
      h[1] = make_double2(is.hit_p.z, is.n.x);
      h[2] = make_double2(is.n.y, is.n.z);
      h[3] = make_double2(is.w_out.x, is.w_out.y);
      h[4] = make_double2(is.w_out.z, qr.t);
    }
    uint4 tail;
    tail.x = RRT_RAY_DISK; tail.y = 0xffffffffu; tail.z = 0xffffffffu; tail.w = qr.steps;
    *reinterpret_cast<uint4*>(h + 5) = tail;
  } else if (hit || qr.captured || !EXIT) {
    store_hit(a, i, hit ? RRT_RAY_HIT : qr.captured ? RRT_RAY_CAPTURED : RRT_RAY_MISS, qr.steps, hit && !ANY, is, qr);
  } else {
    store_exit(a, i, qr.steps, xr);
  }
}
// its launch: camera rays only (a.rays is null)
hipError_t rrt_launch_trace_obs(const KParams* d_kp, const TraceArgs& a, int any, int exit, hipStream_t stream) {
  const uint32_t grid = (a.n - 1u) / 256u + 1u;  // n > 0
#define RRT_GO_O(X, A) hipLaunchKernelGGL((rrt_trace_obs_lane_kernel<X, A>), dim3(grid), dim3(256), 0, stream, d_kp, a)
  if (exit) { if (any) RRT_GO_O(true, true); else RRT_GO_O(true, false); }
  else      { if (any) RRT_GO_O(false, true); else RRT_GO_O(false, false); }
#undef RRT_GO_O
  return hipGetLastError();
}

// the disk kernels' launch: Kerr, lane per ray
hipError_t rrt_launch_trace_disk(const KParams* d_kp, const TraceArgs& a, int any, int exit, hipStream_t stream) {
  const bool cam = a.rays == nullptr;
  const uint32_t grid = (a.n - 1u) / 256u + 1u;  // n > 0
#define RRT_GO_D(X, A, C) hipLaunchKernelGGL((rrt_trace_disk_lane_kernel<X, A, C>), dim3(grid), dim3(256), 0, stream, d_kp, a)
#define RRT_PICK_D(X)                                                       \
  do {                                                                      \
    if (any) { if (cam) RRT_GO_D(X, true, true); else RRT_GO_D(X, true, false); } \
    else     { if (cam) RRT_GO_D(X, false, true); else RRT_GO_D(X, false, false); } \
  } while (0)
  if (exit) RRT_PICK_D(true); else RRT_PICK_D(false);
#undef RRT_PICK_D
#undef RRT_GO_D
  return hipGetLastError();
}

// ------------------------------------------------------------------ launch shim (C++ linkage)
// mode: RRT_TRACE_*; AUTO takes wave-per-ray when every ray can hold a resident wave of its own at
// once -- n <= CUs x the wave kernel's resident waves per CU -- since below that count lane-per-ray
// could not fill the machine anyway (Schwarzschild only; DESIGN.md §5 has the measured crossing).
// *mode_out: the mode launched.
hipError_t rrt_launch_trace(const KParams* d_kp, const TraceArgs& a, int kerr, int any, int exit, int mode, int n_cu,
                            int* mode_out, hipStream_t stream) {
  const bool cam = a.rays == nullptr;
#define RRT_WAVE_K(A, C) rrt_trace_wave_kernel<A, C>
#define RRT_WAVE_X(A, C) rrt_trace_exit_wave_kernel<A, C>
#define RRT_PICK(F, ...)                                          \
  do {                                                            \
    if (any) { if (cam) F(true, true, ##__VA_ARGS__); else F(true, false, ##__VA_ARGS__); } \
    else     { if (cam) F(false, true, ##__VA_ARGS__); else F(false, false, ##__VA_ARGS__); } \
  } while (0)
  if (mode == RRT_TRACE_AUTO) {
    mode = RRT_TRACE_LANE_PER_RAY;
    if (!kerr) {
      int blocks = 0;
      hipError_t e = hipSuccess;
#define RRT_OCC(A, C) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, RRT_WAVE_K(A, C), 256, 0)
#define RRT_OCC_X(A, C) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, RRT_WAVE_X(A, C), 256, 0)
      if (exit) RRT_PICK(RRT_OCC_X); else RRT_PICK(RRT_OCC);
#undef RRT_OCC
#undef RRT_OCC_X
      if (e != hipSuccess) return e;
      if ((uint64_t)a.n <= (uint64_t)n_cu * 4u * (uint64_t)blocks) mode = RRT_TRACE_WAVE_PER_RAY;
    }
  }
  if (mode_out) *mode_out = mode;
  if (mode == RRT_TRACE_WAVE_PER_RAY) {
    const uint32_t grid = (a.n - 1u) / 4u + 1u;  // n > 0
#define RRT_GO(A, C) hipLaunchKernelGGL((RRT_WAVE_K(A, C)), dim3(grid), dim3(256), 0, stream, d_kp, a)
#define RRT_GO_X(A, C) hipLaunchKernelGGL((RRT_WAVE_X(A, C)), dim3(grid), dim3(256), 0, stream, d_kp, a)
    if (exit) RRT_PICK(RRT_GO_X); else RRT_PICK(RRT_GO);
#undef RRT_GO
#undef RRT_GO_X
  } else {
    const uint32_t grid = (a.n - 1u) / 256u + 1u;
#define RRT_GO(A, C, K) hipLaunchKernelGGL((rrt_trace_lane_kernel<K, A, C>), dim3(grid), dim3(256), 0, stream, d_kp, a)
#define RRT_GO_X(A, C, K) hipLaunchKernelGGL((rrt_trace_exit_lane_kernel<K, A, C>), dim3(grid), dim3(256), 0, stream, d_kp, a)
    if (exit) { if (kerr) RRT_PICK(RRT_GO_X, true); else RRT_PICK(RRT_GO_X, false); }
    else if (kerr) RRT_PICK(RRT_GO, true); else RRT_PICK(RRT_GO, false);
#undef RRT_GO
#undef RRT_GO_X
  }
#undef RRT_PICK
#undef RRT_WAVE_K
#undef RRT_WAVE_X
  return hipGetLastError();
}
