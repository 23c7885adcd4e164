// rrt_proof.h -- the proofs that spare a ray (or a pixel's every ray) the exact geodesic march
// (DESIGN.md §5 "The proofs", §10): the planar recurrence and its geometry, stated once, and the shadow,
// Kerr-shadow, camera, rectangle and pixel proofs over them.  A part of rrt_device.h, which includes it
// after query() and the per-sample rules (contraction is off at file scope there); not for use on its own.
#pragma once

namespace rrt {

// ------------------------------------------------------------------ the planar recurrence
// In exact arithmetic the reference's march (next_micro_ray) is planar about the hole and reduces
// to a scalar recurrence: with s = u at a step's start, u' its derivative and v the updated u, the
// step places the next point at c + (cos dt x + sin dt y) / v (flipped through the hole when
// v < 0), and the next step starts from
//   s' = |v| / rho,   u'' = (v cos dt / rho - rho s) / sin dt,   rho = |(cos dt, sin dt)|,
// its x axis = sign(v) E and its y axis = E rotated a quarter turn the same way as y from x,
// E = (cos dt x + sin dt y) / rho.  The reference's floating-point march stays within a relative
// 1e-12 / kappa of that recurrence while no step cancels (|v| >= kappa (|s| + |u' dt|)) --
// measured over 3e5 rays per BASELINE scene (tools/miss_proof_check.py) and on the GPU
// (tests/test_gpu_parity.py).  Launch constants: KParams::miss (rrt_host.cpp fill_proof_params).
// Every helper contracts as the proofs that call it do (the pragma holds per function), and the
// proofs' bits depend on it: which operations fuse decides which borderline rays are proven.
// u'' = f(u) (blackhole.cpp:13-15)
__device__ __forceinline__ double rec_f(const DMissProof& mp, double u) {
#pragma clang fp contract(fast)
  return -u + mp.k15 * u * u;
}
// One row.  vprev: the last v; s: in, the s of the step that made it; out, the next step's start,
// with up its u'.  Returns v: blackhole.cpp:23-32 on (s, u')
__device__ __forceinline__ double rec_row(const DMissProof& mp, const DHole& h, double vprev, double& s, double& up) {
#pragma clang fp contract(fast)
  up = (vprev * mp.co1 - mp.rho * s) * mp.inv_si;
  s = fabs(vprev) * mp.inv_rho;
  const double f1 = rec_f(mp, s);
  const double u2 = s + up * (h.dt * 0.5);
  const double f2 = rec_f(mp, u2);
  const double u3 = u2 + f1 * mp.dt2_4;
  const double f3 = rec_f(mp, u3);
  return s + up * h.dt + (f1 + f2 + f3) * mp.dt2_6;
}
// A cancelling step (or NaN): the recurrence is not certain to follow the reference there
__device__ __forceinline__ bool rec_cancels(const DMissProof& mp, const DHole& h, double s, double up, double v) {
#pragma clang fp contract(fast)
  return !(fabs(v) >= mp.kappa * (s + fabs(up) * h.dt));
}
// The segment A -> B, A = rho E_prev / vprev, B = rho E / v about the hole, with E_prev . E = sg co1
// and |E_prev x E| = si1: its distance from the hole from (vprev, v) alone.  The line through A and
// B lies at distance^2 sin^2 dt / D ...
__device__ __forceinline__ double rec_line_den(const DMissProof& mp, double vprev, double v) {
#pragma clang fp contract(fast)
  return v * v + vprev * vprev - 2.0 * mp.co1 * fabs(vprev) * v;
}
// ... and the segment at the line's where the foot of the perpendicular falls inside it, else at the
// nearer end's, rho^2 / max(v^2, vprev^2).  Is that distance above the radius rb (NaN: no)?  si2 = sin^2 dt
__device__ __forceinline__ bool rec_hole_far(const DMissProof& mp, double si2, double vprev, double v, double rb) {
#pragma clang fp contract(fast)
  const double avp = fabs(vprev);
  const double D = rec_line_den(mp, vprev, v);
  const bool inside = v * (mp.co1 * avp - v) < 0.0 && avp * (avp - mp.co1 * v) > 0.0;
  return inside ? si2 > rb * rb * D : mp.rho * mp.rho > rb * rb * fmax(v * v, vprev * vprev);
}
// A ray's plane about the hole, from its origin o: x = (o - c) / |o - c|, r0 = |o - c|, u0 = 1 / r0 ...
__device__ __forceinline__ v3 ray_axis(v3 c, v3 o, double& r0, double& u0) {
#pragma clang fp contract(fast)
  const v3 x0 = o - c;
  r0 = sqrt(norm2(x0)); u0 = 1.0 / r0;
  return vmul(x0, u0);
}
// ... and its direction d: dx = d . x and y = d - dx x, returned before it is normalised, dy = |y|
__device__ __forceinline__ v3 ray_plane(v3 d, v3 X, double& dx, double& dy) {
#pragma clang fp contract(fast)
  dx = dot(d, X);
  const v3 Y = d - smul(dx, X);
  dy = sqrt(norm2(Y));
  return Y;
}
// The whole march by the recurrence, step 0 included: the ray is the state of a step from the
// point A = o itself (|A - c| = 1 / u0, so v_prev = rho u0, E_prev = x: ea = 1, eb = 0; s_prev
// chosen so the update yields s = u0 and the reference's u' = -u0 (d . x) / |d - (d . x) x|)
__device__ __forceinline__ void rec_start(const DMissProof& mp, const DHole& h, double u0, double dx, double dy, double& vprev, double& s) {
#pragma clang fp contract(fast)
  const double up0 = -u0 * dx / dy;
  vprev = mp.rho * u0;
  s = u0 * mp.co1 - up0 * h.sin_dt * mp.inv_rho;
}

// ------------------------------------------------------------------ shadow-ray occlusion proof
// (DESIGN.md §5).  The reference's shadow query (bvh.cpp:103-113; the caller uses only the
// boolean) is true iff some micro segment before the capture hits a primitive.  Most shadow rays
// of a closed room end on a wall, after ~15-30 exact steps and walks.  The proof marches the
// recurrence from the shadow ray itself (rec_start): every segment must clear the capture sphere by
// the margin m, and once a segment end leaves the trigger box (the root box shrunk past the wall
// triangles kept by rrt_host.cpp build_occluders) the segment must cross one of those triangles with
// margin -- end points m beyond its plane on either side, the crossing point mq inside every edge.
// The reference's segment then crosses it too, its triangle test accepts (triangle.cpp:25-55) and the
// leaf boxes on the way pass, so the query returns true.  Anything else (an end point near a wall, a
// face without triangles, a cancelling step, the march ending) is no proof: the caller marches exactly.
// A certain crossing of one of face f's n[f] wall pieces by the segment a -> b: end points more than m
// on either side of its plane (either way), the crossing point mq inside every edge.  P: the
// shadow proof's triangles (DOccluder, 3 edges) or the Kerr proof's pieces (DOccQuad, 4: a convex quad,
// or a triangle with one edge repeated)
template <class P>
__device__ __forceinline__ bool occ_face(const P (&piece)[6][RRT_OCC_PER_FACE], const uint32_t (&n)[6], int f, v3 a, v3 b, double m) {
#pragma clang fp contract(fast)
  constexpr int E = sizeof(piece[0][0].eo) / sizeof(double);  // edges of a piece
#pragma unroll 1
  for (uint32_t i = 0; i < n[f]; ++i) {
    const P& t = piece[f][i];
    const double da = t.n[0] * a.x + t.n[1] * a.y + t.n[2] * a.z - t.d;
    const double db = t.n[0] * b.x + t.n[1] * b.y + t.n[2] * b.z - t.d;
    if (!((da > m && db < -m) || (da < -m && db > m))) continue;
    const double tq = da / (da - db);
    const v3 q = V(a.x + (b.x - a.x) * tq, a.y + (b.y - a.y) * tq, a.z + (b.z - a.z) * tq);
    // end points within m of the reference's move the crossing by <= m (2 + |b - a| / |da - db|)
    const double mq = m * (2.0 + (fabs(b.x - a.x) + fabs(b.y - a.y) + fabs(b.z - a.z)) / fabs(da - db));
    bool in = true;
    for (int k = 0; k < E; ++k) in = in && t.en[k][0] * q.x + t.en[k][1] * q.y + t.en[k][2] * q.z - t.eo[k] >= mq;
    if (in) return true;
  }
  return false;
}
// The segment a -> b with an end outside the trigger box: 1 = a certain crossing of a wall piece of
// a face that an end is past; -1 = no proof, b has left the root box and the proof gives up there;
// 0 = go on.  QUAD: the Kerr proof's pieces, and it always gives up there; else the shadow proof's
// triangles, and it gives up only without the re-entry rule (kp.shadow_reentry == 0, A/B).  With the
// rule (the default) a ray that has left the room goes on too: a ray thrown out past the hole turns
// round within a few rows (v changes sign, as in the reference's own recurrence) and its next chord
// crosses a wall from outside; occ_face takes either direction, and a chord that comes back through
// a face without triangles continues inside.
// Loops kept rolled: this runs once or twice per shadow ray, and once per row outside the room.
template <bool QUAD>
__device__ __forceinline__ int occ_exit(const KParams& kp, v3 a, v3 b, double m) {
  const DShadowProof& sp = kp.occ;
  // (a segment wholly outside the room meets no kept piece: occ_face's plane test rejects it)
  bool out = false;
#pragma unroll 1
  for (int f = 0; f < 6; ++f) {
    const int k = f < 3 ? f : f - 3;
    const double ak = k == 0 ? a.x : k == 1 ? a.y : a.z, bk = k == 0 ? b.x : k == 1 ? b.y : b.z;
    const bool past = f < 3 ? !(bk >= sp.in_lo[k] && ak >= sp.in_lo[k]) : !(bk <= sp.in_hi[k] && ak <= sp.in_hi[k]);
    if (past && (QUAD ? occ_face(kp.kproof.quad, kp.kproof.nq, f, a, b, m) : occ_face(sp.tri, sp.n, f, a, b, m))) return 1;
    out = out || !(f < 3 ? bk >= kp.miss.lo[k] : bk <= kp.miss.hi[k]);  // NaN: out
  }
  return out && (QUAD || !kp.shadow_reentry) ? -1 : 0;
}
// occ_exit out of line, one copy per kernel build W (inline or the whole proof out of
// line measured slower)
// (an out-of-line callee sees a `const KParams&` as a generic pointer and would read it through
// flat loads: it takes the launch block by its address space and names it generic again inside,
// where the compiler follows the cast; arguments arrive in VGPRs, so the wave-uniform address goes
// to SGPRs first and the reads take the scalar path)
template <int W>
__device__ __noinline__ int occ_exit_call(const RRT_CONST_AS KParams* kpq, v3 a, v3 b, double m) {
  return occ_exit<false>(*(const KParams*)uniform_ptr(kpq), a, b, m);
}
__device__ __forceinline__ bool occ_inside(const DShadowProof& sp, v3 b) {
  return b.x >= sp.in_lo[0] && b.x <= sp.in_hi[0] && b.y >= sp.in_lo[1] && b.y <= sp.in_hi[1] && b.z >= sp.in_lo[2] &&
         b.z <= sp.in_hi[2];
}
// Kerr shadow rays ("Kerr occlusion proof").  A shadow query is true iff some
// segment of the march before the capture hits a primitive; from inside a closed room most end on
// a wall after 20-60 RK4 steps, each step four Hamiltonian evaluations plus a walk.  The proof
// marches the same Hamiltonian with steps kp.kproof.stretch times longer and accepts "occluded"
// when one of its chords crosses a wall piece (build_occluders: kp.occ's triangles, coplanar pairs
// merged into convex quads, kp.kproof.quad) with margin delta:
// end points more than delta on either side of the plane, the crossing point inside every edge by
// occ_face's mq.  The exact march's chords stay within delta of the coarse chords while the coarse
// march keeps sqrt(r_near2) from the hole (tools/kerr_proof_sweep.py: the largest deviation seen
// over the envelope rrt_host.cpp allows is under a third of delta), so they cross that triangle
// too, uncaptured (the coarse path, and so the exact one, stays far outside the horizon) and
// within the exact march's budget (max_steps coarse steps, swept angle below swept_max); the
// triangle test accepts and the leaf boxes on the way contain the crossing, so the query is true.
// Anything else -- near the hole, the ray leaving the room, an operand outside the fast cores'
// range, the budget -- is no proof: the exact march runs.
// A ray whose straight line leaves the room through a face without wall pieces (the open side of a
// Cornell box) almost never ends on a wall: spare it the coarse march (false: no proof)
__device__ __forceinline__ bool kerr_proof_worth(const KParams& kp, v3 o, v3 d) {
  double te = 1e300;
  int fe = -1;
  for (int k = 0; k < 3; ++k) {
    const double dk = k == 0 ? d.x : k == 1 ? d.y : d.z, ok = k == 0 ? o.x : k == 1 ? o.y : o.z;
    if (dk == 0.0) continue;
    const double t = ((dk > 0.0 ? kp.miss.hi[k] : kp.miss.lo[k]) - ok) / dk;
    if (t < te) { te = t; fe = dk > 0.0 ? k + 3 : k; }
  }
  return !(fe >= 0 && kp.kproof.nq[fe] == 0);
}
__device__ __forceinline__ bool kerr_occluded_proof(const KParams& kp, v3 o, v3 d) {
  const DHole& h = kp.hole;
  const DKerrProof& kq = kp.kproof;
  if (!kerr_proof_worth(kp, o, d)) return false;
  v3 q, p;
  kerr_init(h, o, d, q, p);
  if (!(norm2(q) > kq.r_near2)) return false;  // starting near the hole
  const v3 c = ld3(h.c);
  v3 a = o, a0 = o;  // the chord's start, and the previous chord's
  bool a_in = occ_inside(kp.occ, a);
  double swept = 0.0;
#pragma unroll 1
  for (int j = 0; j < kq.max_steps; ++j) {
    KArith<true> ar;
    const bool escaped = kerr_advance(h, q, p, swept, ar, kq.stretch);
    if (!ar.ok || escaped || !(swept < kq.swept_max) || !(norm2(q) > kq.r_near2)) return false;
    const v3 b = kerr_world(h, q);
    {  // the chord keeps sqrt(r_near2) from the hole too
      const v3 u = b - a, w = c - a;
      const double uu = norm2(u), t = uu > 0.0 ? fmin(fmax(dot(u, w) / uu, 0.0), 1.0) : 0.0;
      if (!(norm2(w - vmul(u, t)) > kq.r_near2)) return false;
    }
    const bool b_in = occ_inside(kp.occ, b);
    if (!b_in || !a_in) {
      int res = occ_exit<true>(kp, a, b, kq.delta);
      if (res <= 0 && j > 0) {
        // a wall crossed across two chords (one of their common point's sides within delta of the
        // plane): the chord a0 -> b, with the margin grown by a's distance from it
        const v3 u = b - a0, w = a - a0;
        const double uu = norm2(u), uw = dot(u, w);
        const double beta = sqrt(fmax(norm2(w) - uw * uw / uu, 0.0)) * (1.0 + 1e-6);
        if (uu > 0.0 && occ_exit<true>(kp, a0, b, kq.delta + beta) > 0) res = 1;
      }
      if (res) return res > 0;
    }
    a_in = b_in;
    a0 = a;
    a = b;
  }
  return false;
}
// The whole march by the recurrence, step 0 included, from the point A = o itself.
// (This function restates ray_axis, ray_plane, rec_start, rec_row, rec_cancels and rec_hole_far inline:
// through the start's helpers or through the row's, every kernel that holds this proof spilled two or
// more SGPRs more than with the text here, rrt_batch_kernel<1, 4> 167 for 155,
// profiles/proof_rules_isa.txt.  A change to one of those helpers is made here too.)
template <int W = 0>
__device__ __forceinline__ bool shadow_occluded_proof(const KParams& kp, v3 o, v3 d, int steps) {
#pragma clang fp contract(fast)
  const DMissProof& mp = kp.miss;
  const DShadowProof& sp = kp.occ;
  const DHole& h = kp.hole;
  const v3 c = V(h.c[0], h.c[1], h.c[2]);
  const v3 x0 = o - c;
  const double r0 = sqrt(norm2(x0)), u0 = 1.0 / r0;
  const v3 X = vmul(x0, u0);
  const double dx = dot(d, X);
  v3 Y = d - smul(dx, X);
  const double dy = sqrt(norm2(Y));
  Y = vmul(Y, 1.0 / dy);
  const double up0 = -u0 * dx / dy;
  double vprev = mp.rho * u0, s = u0 * mp.co1 - up0 * h.sin_dt * mp.inv_rho;
  double ea = 1.0, eb = 0.0, sig = 1.0, rp = r0;
  bool a_in = occ_inside(sp, o);
  const double si2 = h.sin_dt * h.sin_dt, rc = h.r * (1.0 + 1e-9);
#pragma unroll 1
  for (int j = 0; j < steps; ++j) {
    const double sg = vprev < 0.0 ? -1.0 : 1.0;
    const double up = (vprev * mp.co1 - mp.rho * s) * mp.inv_si;
    s = fabs(vprev) * mp.inv_rho;
    const double f1 = -s + mp.k15 * s * s;
    const double u2 = s + up * (h.dt * 0.5);
    const double f2 = -u2 + mp.k15 * u2 * u2;
    const double u3 = u2 + f1 * mp.dt2_4;
    const double f3 = -u3 + mp.k15 * u3 * u3;
    const double v = s + up * h.dt + (f1 + f2 + f3) * mp.dt2_6;
    if (!(fabs(v) >= mp.kappa * (s + fabs(up) * h.dt))) return false;  // cancelling step (or NaN)
    const double a = sg * mp.co1, b = sig * mp.si1;
    const double na = a * ea - b * eb, nb = a * eb + b * ea;
    sig *= sg;
    const double av = fabs(v), avp = fabs(vprev);
    const double r = mp.rho * __builtin_amdgcn_rcp(av) * (1.0 + 1e-6);  // |B - c| (upper bound)
    const double m = mp.eta * (fmax(rp, r) + mp.scale);
    // the segment must clear the capture sphere: its distance from the hole > r_s + m (the
    // camera proof's scalar distance: foot of the perpendicular inside, else the nearer end)
    const double rb = rc + m;
    const double D = v * v + vprev * vprev - 2.0 * mp.co1 * avp * v;
    const bool inside = v * (mp.co1 * avp - v) < 0.0 && avp * (avp - mp.co1 * v) > 0.0;
    const bool clear = inside ? si2 > rb * rb * D : mp.rho * mp.rho > rb * rb * fmax(v * v, vprev * vprev);
    if (!clear) return false;
    const double ib = mp.rho / v;
    const v3 pb = V(c.x + (na * ib) * X.x + (nb * ib) * Y.x, c.y + (na * ib) * X.y + (nb * ib) * Y.y,
                    c.z + (na * ib) * X.z + (nb * ib) * Y.z);
    const bool b_in = occ_inside(sp, pb);
    if (!b_in || !a_in) {
      const double ia = mp.rho / vprev;
      const v3 pa = V(c.x + (ea * ia) * X.x + (eb * ia) * Y.x, c.y + (ea * ia) * X.y + (eb * ia) * Y.y,
                      c.z + (ea * ia) * X.z + (eb * ia) * Y.z);
      const int res = occ_exit_call<W>((const RRT_CONST_AS KParams*)&kp, pa, pb, m);
      if (res) return res > 0;
    }
    a_in = b_in;
    rp = r; vprev = v; ea = na; eb = nb;
  }
  return false;
}

// ------------------------------------------------------------------ camera-ray miss proof
// (DESIGN.md §5 "Miss proof").  A segment of the recurrence that misses the root box widened
// by eta (|P - c| + scale), eta >= 1e3 x the recurrence's deviation bound, is a reference segment
// whose root slab test fails.  If every segment misses, the reference's query returns "no hit"
// (captured or not), so the camera ray is a miss without the exact march.  Step 0 is the
// reference's own step (bit exact) and its segment takes the reference's root test.  Any doubt (a
// cancelling step, a segment near the box, NaN) returns false: the caller marches the ray exactly.
__device__ __forceinline__ bool seg_clear_of_box(v3 a, v3 b, const double* lo, const double* hi, double m) {
#pragma clang fp contract(fast)
  const double l0 = lo[0] - m, l1 = lo[1] - m, l2 = lo[2] - m, h0 = hi[0] + m, h1 = hi[1] + m, h2 = hi[2] + m;
  if (fmax(a.x, b.x) < l0 || fmin(a.x, b.x) > h0 || fmax(a.y, b.y) < l1 || fmin(a.y, b.y) > h1 ||
      fmax(a.z, b.z) < l2 || fmin(a.z, b.z) > h2)
    return true;
  // slab test of the segment a + t (b - a), t in [0, 1]; every axis overlaps the widened box here,
  // so an axis with no extent along the segment constrains nothing
  const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  double tmin = 0.0, tmax = 1.0;
  if (dx != 0.0) { const double i = 1.0 / dx, t0 = (l0 - a.x) * i, t1 = (h0 - a.x) * i; tmin = fmax(tmin, fmin(t0, t1)); tmax = fmin(tmax, fmax(t0, t1)); }
  if (dy != 0.0) { const double i = 1.0 / dy, t0 = (l1 - a.y) * i, t1 = (h1 - a.y) * i; tmin = fmax(tmin, fmin(t0, t1)); tmax = fmin(tmax, fmax(t0, t1)); }
  if (dz != 0.0) { const double i = 1.0 / dz, t0 = (l2 - a.z) * i, t1 = (h2 - a.z) * i; tmin = fmax(tmin, fmin(t0, t1)); tmax = fmin(tmax, fmax(t0, t1)); }
  return tmin > tmax + 1e-9;  // NaN: not clear
}
template <bool COUNT = false>
__device__ __forceinline__ bool camera_miss_proof(const KParams& kp, v3 o, v3 d, Counters& cn) {
  const DMissProof& mp = kp.miss;
  const DHole& h = kp.hole;
  // step 0: the reference's own step from the camera ray (bit exact) and its root slab test
  MicroOut m0;
  v3 rel;
  double rel2, max_t = 0.0;
  next_micro_at(h, o + vmul(d, max_t), o, d, max_t, rel, rel2, &m0);
  const v3 e = o + vmul(d, max_t);
  if (!segment_outside_root(kp, o, e)) {
    const v3 y = V(xdiv(1.0, d.x), xdiv(1.0, d.y), xdiv(1.0, d.z));
    if (COUNT) cn.bbox++;
    if (slab_rt(kp.nodes[0].mn, kp.nodes[0].mx, o, d, y, max_t, !segment_fast(kp, o, d))) return false;
  }
  {
#pragma clang fp contract(fast)
    const v3 c = V(h.c[0], h.c[1], h.c[2]);
    const v3 X = m0.x, Y = m0.y;
    double s = m0.u, up = m0.up, vprev = m0.v;
    double ea = mp.co1, eb = mp.si1, sig = 1.0;  // E of the point just placed, in (X, Y); sense of y from x
    double rp = mp.rho / fabs(vprev);             // its distance from the hole
    const double si2 = h.sin_dt * h.sin_dt;
    for (int j = 1; j < h.steps; ++j) {
      const double sg = vprev < 0.0 ? -1.0 : 1.0;
      const double v = rec_row(mp, h, vprev, s, up);
      if (rec_cancels(mp, h, s, up, v)) return false;
      // E of the new point: cos dt x + sin dt y over rho, with x = sg E_prev, y = sig-turned E_prev
      const double a = sg * mp.co1, b = sig * mp.si1;
      const double na = a * ea - b * eb, nb = a * eb + b * ea;
      sig *= sg;
      const double r = mp.rho * __builtin_amdgcn_rcp(fabs(v)) * (1.0 + 1e-6);  // |B| (upper bound)
      const double rb = mp.r_ball + mp.eta * (fmax(rp, r) + mp.scale);
      if (!rec_hole_far(mp, si2, vprev, v, rb)) {
        // within reach of the root box: the segment itself against the widened box
        const double ia = mp.rho / vprev, ib = mp.rho / v;
        const v3 pa = V(c.x + (ea * ia) * X.x + (eb * ia) * Y.x, c.y + (ea * ia) * X.y + (eb * ia) * Y.y,
                        c.z + (ea * ia) * X.z + (eb * ia) * Y.z);
        const v3 pb = V(c.x + (na * ib) * X.x + (nb * ib) * Y.x, c.y + (na * ib) * X.y + (nb * ib) * Y.y,
                        c.z + (na * ib) * X.z + (nb * ib) * Y.z);
        if (!seg_clear_of_box(pa, pb, mp.lo, mp.hi, mp.eta * (fmax(rp, r) + mp.scale))) return false;
      }
      rp = r; vprev = v; ea = na; eb = nb;
    }
  }
  return true;
}
// Is the camera ray (o, d) a proven miss?  Schwarzschild builds only; the reference-work
// counting passes (COUNT without count_exec) always march exactly.
// W: the calling kernel build's tag -- one copy per build, since a callee shared by builds of
// different waves-per-SIMD budgets takes the smallest budget's registers for all of them
template <bool COUNT, int W>
__device__ __noinline__ bool camera_miss_proof_call(const RRT_CONST_AS KParams* kpq, v3 o, v3 d, Counters& cn) {
  return camera_miss_proof<COUNT>(*(const KParams*)uniform_ptr(kpq), o, d, cn);
}
// NI: out of line (the register-heavy per-pixel-loop builds keep their occupancy), W its build tag
template <bool COUNT, bool KERR, bool NI = false, int W = 0>
__device__ __forceinline__ bool camera_proven_miss(const KParams& kp, v3 o, v3 d, Counters& cn) {
  if (KERR || !kp.miss.on || (COUNT && !kp.count_exec)) return false;
  RRT_T0(tp0);
  const bool r = NI ? camera_miss_proof_call<COUNT, W>((const RRT_CONST_AS KParams*)&kp, o, d, cn)
                    : camera_miss_proof<COUNT>(kp, o, d, cn);
  RRT_ACC(t_proof, tp0);
  if (COUNT && r && kp.audit && audit_pick(kp, o, d)) {
    Counters c2 = {};
    Isect i2;
    audit_note(kp, RRT_AUDIT_CAMERA, query<false, false, false>(kp, o, d, &i2, c2));
  }
  return r;
}

// ------------------------------------------------------------------ pixel miss proof
// (DESIGN.md §5).  Every camera ray of pixel (px, py) -- jitter anywhere in the pixel's square,
// part1_code.cpp:182-187 -- is a proven miss.  All the rays start at the camera position O, so
// they share x = (O - c) / |O - c| and u = 1 / |O - c|; a ray's planar march depends on its
// direction only through dx = d . x (u' = -u dx / sqrt(1 - dx^2)), and its plane only through
// y.  The proof runs the recurrence for the pixel's least, central and largest dx (from its
// corners and centre, widened for curvature) and, while the three agree in the sign of every v
// and vary little, bounds every ray's points around the central ray's: with the frame (ea, eb)
// the same for all, |P - P_c| <= rho |1/v - 1/v_c| + (rho / |v|) |eb| |y - y_c|.  Each segment
// of the central ray must then clear the root box by the camera proof's margin plus that bound.
// Launch constants are the camera proof's (KParams::miss) and the camera's.
// A rectangle of pixels (the strip pass, rrt_strip_proof_kernel): jitter positions [px, px + w] x
// [py, py + h]; the same argument with the rectangle's corners and centre (the curvature term
// uses its half-diagonal, so it holds for any small rectangle; w = h = 1 is pixel_miss_proof).
__device__ __forceinline__ bool rect_miss_proof(const KParams& kp, double px, double py, double w, double hgt) {
#pragma clang fp contract(fast)
  const DMissProof& mp = kp.miss;
  const DHole& h = kp.hole;
  const v3 O = ld3(kp.cam.pos), c = ld3(h.c);
  double r0, u0, dxc, dyc;
  const v3 X = ray_axis(c, O, r0, u0);
  // the pixel's directions: dx range, the centre's plane axis y_c and the spread of y
  const v3 dc = pixel_ray_dir(kp, px + 0.5 * w, py + 0.5 * hgt);
  v3 Yc = ray_plane(dc, X, dxc, dyc);
  if (!(dyc > 1e-3)) return false;  // towards the hole: no stable plane
  Yc = vmul(Yc, 1.0 / dyc);
  double dlo = dxc, dhi = dxc, dY = 0.0, dd = 0.0, dymin = dyc;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const v3 d = pixel_ray_dir(kp, px + (k & 1) * w, py + (k >> 1) * hgt);
    double dx, dy;
    const v3 yv = ray_plane(d, X, dx, dy);
    dlo = fmin(dlo, dx);
    dhi = fmax(dhi, dx);
    if (!(dy > 1e-3)) return false;
    dymin = fmin(dymin, dy);
    dY = fmax(dY, sqrt(norm2(vmul(yv, 1.0 / dy) - Yc)));
    dd = fmax(dd, sqrt(norm2(d - dc)));
  }
  // Every direction of the rectangle lies within dd of dc (the farthest point of a convex spherical
  // polygon from an inner point is a vertex), so the directions +-X -- where the plane axis y turns
  // round -- stay outside it when dd is well below the sine of dc's angle from them, and y then
  // varies smoothly over the rectangle, its spread set by the corners.  A rectangle subtending a
  // large angle near +-X (small frames, wide fields of view) is left to the pixel level.
  if (!(dd <= 0.25 * dymin)) return false;
  // a smooth function over the small square: extremes within the corners' values plus a
  // curvature term of the square's angular radius squared
  const double slack = 2.0 * dd * dd + 1e-12, wdx = dhi - dlo;
  dlo -= 0.05 * wdx + slack;
  dhi += 0.05 * wdx + slack;
  dY = 1.25 * dY + slack;
  if (!(dlo > -1.0 && dhi < 1.0)) return false;
  // three planar recurrences (least, central, largest dx), started at A = O (rec_start)
  double s[3], vp[3];
  {
    const double dxs[3] = {dlo, dxc, dhi};
#pragma unroll
    for (int i = 0; i < 3; ++i) rec_start(mp, h, u0, dxs[i], sqrt(1.0 - dxs[i] * dxs[i]), vp[i], s[i]);
  }
  double ea = 1.0, eb = 0.0, sig = 1.0, rp = r0, dpa = 0.0, dvp = 0.0;  // A = O: the same for all rays
  const double si2 = h.sin_dt * h.sin_dt;
#pragma unroll 1
  for (int j = 0; j < h.steps; ++j) {
    double v[3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double up;
      v[i] = rec_row(mp, h, vp[i], s[i], up);
      ok = ok && !rec_cancels(mp, h, s[i], up, v[i]);
    }
    // one sign history for the whole pixel, and v far from 0 compared with its spread
    const double dv = 1.5 * fmax(fabs(v[0] - v[1]), fabs(v[2] - v[1]));
    const double av = fabs(v[1]);
    if (!(ok && (v[0] < 0.0) == (v[1] < 0.0) && (v[2] < 0.0) == (v[1] < 0.0) && av > 2.0 * dv)) return false;
    const double sg = vp[1] < 0.0 ? -1.0 : 1.0;
    const double a = sg * mp.co1, b = sig * mp.si1;
    const double na = a * ea - b * eb, nb = a * eb + b * ea;
    sig *= sg;
    const double r = mp.rho / (av - dv) * (1.0 + 1e-6);  // |B - c| over the pixel (upper bound)
    const double dpb = mp.rho * dv / (av * (av - dv)) * (1.0 + 1e-6) + r * fabs(nb) * dY;
    const double m0 = mp.eta * (fmax(rp, r) + mp.scale);
    const double m = m0 + fmax(dpa, dpb);
    // Distance from the hole: a ray's segment depends only on its (v_prev, v) -- turning the
    // plane about x keeps it -- and the pixel's pairs lie in [v_prev +- dvp] x [v +- dv], a box
    // on which neither coordinate changes sign (checked above, and for v_prev one step earlier).
    // A segment is never nearer the hole than its line (rec_line_den: distance^2 sin^2 dt / D), and
    // D is a positive definite quadratic form on that box (convex: its maximum, the nearest line, at
    // a corner), so the line test at the four corners covers every ray of the pixel, whichever
    // side of its segment the foot of the perpendicular falls on.
    const double rb = mp.r_ball + m0;
    bool far = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double w = v[1] + ((k & 1) ? dv : -dv), wp = vp[1] + ((k & 2) ? dvp : -dvp);
      far = far && si2 > rb * rb * rec_line_den(mp, wp, w);
    }
    // Separating half-space: in a ray's own plane (coordinates about the hole on X and
    // its axis Y) the segment runs from a eA to b eB, eA = sg (ea, eb) and eB = sign(v) (na, nb) the
    // same for every ray of the rectangle (one sign history), a in [rho / (|vp| + dvp), rp] and b in
    // [rho / (av + dv), r].  With n the central segment's in-plane unit normal, n . eA > 0 and
    // n . eB > 0, every point of every such segment has n-coordinate >= dmin (a convex combination of
    // its ends).  In space n3 = n_x X + n_y Yc: a point alpha X + beta Y has n3 . (P - c) = alpha n_x +
    // beta n_y (Y . Yc) >= alpha n_x + beta n_y - |beta| dY^2 / 2, |beta| at most at an end.  The
    // box's support about the hole in direction n3 is hs, the widening by m0 on every axis adds at
    // most sqrt(3) m0 to it: a row with dmin beyond both is clear of the widened box.  Rows j >= 1;
    // anything else (NaN included) falls through to the slab test.
    if (!far && kp.halfspace && j >= 1) {
      const double sv = v[1] < 0.0 ? -1.0 : 1.0, avp = fabs(vp[1]);
      const double eax = sg * ea, eay = sg * eb, ebx = sv * na, eby = sv * nb;
      const double ac = mp.rho / avp, bc = mp.rho / av;
      const double tx = bc * ebx - ac * eax, ty = bc * eby - ac * eay;
      const double it = 1.0 / sqrt(tx * tx + ty * ty);
      double nx = -ty * it, ny = tx * it, gA = nx * eax + ny * eay;
      if (gA < 0.0) { nx = -nx; ny = -ny; gA = -gA; }
      const double gB = nx * ebx + ny * eby;
      const double dmin = fmin(mp.rho / (avp + dvp) * gA, mp.rho / (av + dv) * gB);
      const double bmax = fmax(rp * fabs(eb), r * fabs(nb));
      const v3 n3 = smul(nx, X) + smul(ny, Yc);
      const double hs = fmax(n3.x * (mp.lo[0] - c.x), n3.x * (mp.hi[0] - c.x)) +
                        fmax(n3.y * (mp.lo[1] - c.y), n3.y * (mp.hi[1] - c.y)) +
                        fmax(n3.z * (mp.lo[2] - c.z), n3.z * (mp.hi[2] - c.z));
      far = gA > 0.0 && gB > 0.0 && dmin * (1.0 - 1e-6) - bmax * (0.5 * dY * dY) > hs + 3.0 * m0;
    }
    if (!far) {
      const double ia = mp.rho / vp[1], ib = mp.rho / v[1];
      const v3 pa = j == 0 ? O : V(c.x + (ea * ia) * X.x + (eb * ia) * Yc.x, c.y + (ea * ia) * X.y + (eb * ia) * Yc.y,
                                   c.z + (ea * ia) * X.z + (eb * ia) * Yc.z);
      const v3 pb = V(c.x + (na * ib) * X.x + (nb * ib) * Yc.x, c.y + (na * ib) * X.y + (nb * ib) * Yc.y,
                      c.z + (na * ib) * X.z + (nb * ib) * Yc.z);
      if (!seg_clear_of_box(pa, pb, mp.lo, mp.hi, m)) return false;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) vp[i] = v[i];
    rp = r; dpa = dpb; dvp = dv; ea = na; eb = nb;
  }
  return true;
}
__device__ __forceinline__ bool pixel_miss_proof(const KParams& kp, uint32_t px, uint32_t py) {
  return rect_miss_proof(kp, (double)px, (double)py, 1.0, 1.0);
}

// Heavy pixel (slot-parallel heavy pixels): some of the pixel's rays are captured
// by the hole and some not, or its rays pass within sqrt(kp.heavy_r2) of the hole.  Such pixels
// orbit the hole before they reach the geometry (the costliest queries of a frame) and mix hits
// with misses (several speculation rounds per step in the batch kernel), so their slots are
// rendered in parallel by whole batch-kernel waves (rrt_sample.hip heavy_pixel_wave).  A routing
// heuristic only -- the pixel's result is the same on either path.  The planar recurrence for the
// least and largest dx of the pixel's corners; a segment's distance from the hole follows from
// (v_prev, v) alone, here against two radii and with the test the other way round.
// (This function restates ray_axis, rec_start, rec_row, rec_line_den and rec_hole_far's distance inline:
// through them rrt_pixel_proof_kernel came out 29 instructions longer, profiles/proof_rules_isa.txt.)
__device__ __forceinline__ bool pixel_heavy(const KParams& kp, uint32_t px, uint32_t py) {
#pragma clang fp contract(fast)
  const DMissProof& mp = kp.miss;
  const DHole& h = kp.hole;
  const v3 O = ld3(kp.cam.pos), c = ld3(h.c);
  const v3 x0 = O - c;
  const double r0 = sqrt(norm2(x0)), u0 = 1.0 / r0;
  const v3 X = vmul(x0, u0);
  double dlo = 2.0, dhi = -2.0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const double dx = dot(pixel_ray_dir(kp, (double)px + (k & 1), (double)py + (k >> 1)), X);
    dlo = fmin(dlo, dx);
    dhi = fmax(dhi, dx);
  }
  if (!(dlo > -1.0 && dhi < 1.0)) return true;  // looking at the hole
  const double r2 = h.r2, near2 = kp.heavy_r2, si2 = h.sin_dt * h.sin_dt, rho2 = mp.rho * mp.rho;
  bool cap[2] = {false, false}, close = false;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double dx = i ? dhi : dlo;
    const double up0 = -u0 * dx / sqrt(1.0 - dx * dx);
    double vp = mp.rho * u0, s = u0 * mp.co1 - up0 * h.sin_dt * mp.inv_rho;
#pragma unroll 1
    for (int j = 0; j < h.steps; ++j) {
      const double up = (vp * mp.co1 - mp.rho * s) * mp.inv_si;
      s = fabs(vp) * mp.inv_rho;
      const double f1 = -s + mp.k15 * s * s;
      const double u2 = s + up * (h.dt * 0.5);
      const double f2 = -u2 + mp.k15 * u2 * u2;
      const double u3 = u2 + f1 * mp.dt2_4;
      const double f3 = -u3 + mp.k15 * u3 * u3;
      const double v = s + up * h.dt + (f1 + f2 + f3) * mp.dt2_6;
      const double av = fabs(v), avp = fabs(vp);
      const double D = v * v + vp * vp - 2.0 * mp.co1 * avp * v;
      const bool inside = v * (mp.co1 * avp - v) < 0.0 && avp * (avp - mp.co1 * v) > 0.0;
      // distance^2 from the hole below d2  <=>  inside ? si2 / D : rho^2 / max(v, vp)^2 below d2
      const double m2 = fmax(v * v, vp * vp);
      const bool in_r = inside ? si2 < r2 * D : rho2 < r2 * m2;
      const bool in_n = inside ? si2 < near2 * D : rho2 < near2 * m2;
      close = close || in_n;
      if (in_r) { cap[i] = true; break; }
      if (!(av > 0.0)) break;  // NaN or a degenerate step
      vp = v;
    }
  }
  return cap[0] != cap[1] || (close && !(cap[0] && cap[1]));
}

// W: the occlusion proof's build tag (0: no proof in this build).  Its out-of-line part (the face
// test, occ_exit_call) gets one copy per calling kernel build: a callee shared by kernels of
// different waves-per-SIMD budgets gets the smallest budget's registers, and every caller then
// allocates the callee's count.  Measured on cfg3 (profiles/r02_ab_log.md): inline 31.5 ms, face
// test out of line 31.3, whole proof out of line 37.6 (the call's frame and SGPR saves), no proof
// 35.3.
template <bool ANY, bool COUNT, bool KERR = false, int W = 0, bool W4 = true, bool SCOPED = false>
__device__ __forceinline__ bool query_nx(const KParams& kp, v3 o, v3 d, Isect* is, Counters& cn) {
  // shadow rays: the occlusion proof first (Schwarzschild; never in the reference-work counts)
  if (W && ANY && !KERR && kp.occ.on && !(COUNT && !kp.count_exec)) {
    RRT_T0(tp0);
    const KParams& kq = kp_stage<SCOPED>(kp);  // the proof's constants: live inside it only
    const bool occluded = shadow_occluded_proof<W>(kq, o, d, kq.hole.steps);
    RRT_ACC(t_squery, tp0);
    RRT_ACC(t_sproof, tp0);
    if (occluded) {
      if (COUNT && kp.audit && audit_pick(kp, o, d)) {
        Counters c2 = {};
        audit_note(kp, RRT_AUDIT_SHADOW, !query<true, false, false>(kp, o, d, nullptr, c2));
      }
      return true;
    }
  }
  return query<ANY, COUNT, KERR, W4, false, false, false, false, SCOPED>(kp, o, d, is, cn);
}


}  // namespace rrt
