"""The CPU rule of the thin accretion disk (rrt_set_disk, RRT_RAY_DISK), restated from
DESIGN.md §12 in IEEE double with the operations in the order fixed there (Python floats: one
correctly rounded operation at a time, no contraction).

It works from the rows of the restated Kerr march (oracle_lib.kerr_chain_st: chord o3, d3, max_t, the
capture flag, and the local state q3, p3 after the step; the swept angle after the step), plus a
restatement of kerr_init for the state (q0, p0) the first step starts from.  For one ray it gives every
crossing of the plane z = 0, the first crossing on the annulus with s, the crossing point, L_z, g and
the radiance, and -- from the ray's checked disk-less record -- the record the disk-aware march must
return.
"""
import math

import numpy as np

import exit_check as xc
import oracle_lib as ol
import rrt
import trace_check as tc

MISS, HIT, CAPTURED, ESCAPED, DISK = (rrt.RRT_RAY_MISS, rrt.RRT_RAY_HIT, rrt.RRT_RAY_CAPTURED, rrt.RRT_RAY_ESCAPED,
                                      rrt.RRT_RAY_DISK)


def isco(spin):
    """Prograde ISCO radius in M (Bardeen, Press & Teukolsky 1972)."""
    z1 = 1.0 + np.cbrt(1.0 - spin * spin) * (np.cbrt(1.0 + spin) + np.cbrt(1.0 - spin))
    z2 = math.sqrt(3.0 * spin * spin + z1 * z1)
    return 3.0 + z2 - math.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2))


class Hole:
    """bh = (cx, cy, cz, r_s, dtheta), kerr = (spin, axis): M, a, the local frame (the restatement's)."""

    def __init__(self, bh, kerr):
        self.bh, self.kerr = tuple(bh), kerr
        self.c = [float(v) for v in bh[:3]]
        self.m = 0.5 * float(bh[3])
        self.a = float(kerr[0]) * self.m
        self.a2 = self.a * self.a
        _, fr = ol.kerr_chain(self.bh, kerr[0], kerr[1], (self.c[0] + 1.0, self.c[1] + 2.0, self.c[2] + 3.0),
                              (1.0, 0.0, 0.0), max_rows=1)
        self.ex, self.ey, self.ez = ([float(v) for v in fr[i]] for i in range(3))
        self.max_steps = 4 * tc.steps_of(bh[4])

    def local(self, v):
        return [v[0] * e[0] + v[1] * e[1] + v[2] * e[2] for e in (self.ex, self.ey, self.ez)]


class Disk:
    """The device constants of a disk (rrt_host.cpp fill_disk_params): r_in, r_out in M (r_in resolved:
    take it from rrt_get_disk), emission float32 [3]."""

    def __init__(self, hole, r_in, r_out, emission=(1.0, 1.0, 1.0), redshift=True):
        self.r_in_m, self.r_out_m = float(r_in), float(r_out)
        self.r_in = float(r_in) * hole.m
        self.r_in2 = self.r_in * self.r_in
        ro = float(r_out) * hole.m
        self.r_out2 = ro * ro
        self.sqrt_m = math.sqrt(hole.m)
        self.k = hole.a * self.sqrt_m
        self.emission = np.asarray(emission, np.float32)
        self.redshift = bool(redshift)


def kerr_init(hole, o, d):
    """rrt_device.h kerr_init / kerr_fl: the local position q and covector p (p_t = -1) of a photon at
    world point o moving along world direction d."""
    h = hole
    q = h.local([float(o[i]) - h.c[i] for i in range(3)])
    k = h.local([float(v) for v in d])
    zz = q[2] * q[2]
    w = ((q[0] * q[0] + q[1] * q[1]) + zz) - h.a2
    r2 = 0.5 * w + math.sqrt(0.25 * (w * w) + h.a2 * zz)
    r = math.sqrt(r2)
    iw = 1.0 / (r2 + h.a2)
    l = [(r * q[0] + h.a * q[1]) * iw, (r * q[1] - h.a * q[0]) * iw, q[2] / r]
    f = ((2.0 * h.m) * (r * r2)) / (r2 * r2 + h.a2 * zz)
    ld = (l[0] * k[0] + l[1] * k[1]) + l[2] * k[2]
    A, B, C = f - 1.0, 2.0 * f * ld, 1.0 + f * (ld * ld)
    disc = B * B - 4.0 * A * C
    if not disc > 0.0:
        disc = 0.0
    kt = (2.0 * C) / (math.sqrt(disc) - B)
    pt = A * kt + f * ld
    s = f * (kt + ld)
    p = [k[i] + s * l[i] for i in range(3)]
    if pt < 0.0:
        c = -1.0 / pt
        p = [p[i] * c for i in range(3)]
    return q, p


def hamiltonian(hole, q, p):
    """(H, |p|^2) of the Kerr-Schild photon Hamiltonian H = (|p|^2 - 1 - f (1 + l . p)^2) / 2 at p_t = -1."""
    h = hole
    zz = q[2] * q[2]
    w = q[0] * q[0] + q[1] * q[1] + zz - h.a2
    r2 = 0.5 * w + math.sqrt(0.25 * w * w + h.a2 * zz)
    r = math.sqrt(r2)
    l = [(r * q[0] + h.a * q[1]) / (r2 + h.a2), (r * q[1] - h.a * q[0]) / (r2 + h.a2), q[2] / r]
    f = 2.0 * h.m * r * r2 / (r2 * r2 + h.a2 * zz)
    L = 1.0 + l[0] * p[0] + l[1] * p[1] + l[2] * p[2]
    pp = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
    return 0.5 * (pp - 1.0 - f * L * L), pp


class Crossing:
    """One crossing of the plane: row, s, local x, y, r2 = x^2 + y^2 - a^2, on (the annulus), side (+1: the
    ray came from z > 0), and for a crossing on the annulus t, hit_p, w_out, lz, g, w, rgb, n."""


def redshift(hole, disk, r, lz):
    r32 = r * math.sqrt(r)
    kr = disk.k / r32
    om = disk.sqrt_m / (r32 + disk.k)
    ut = (1.0 + kr) / math.sqrt((1.0 - (3.0 * hole.m) / r) + 2.0 * kr)
    den = ut * (1.0 - om * lz)
    g = 1.0 / den if den != 0.0 else math.inf
    if not (g > 0.0 and math.isfinite(g)):
        g = 0.0
    return g


def crossings(hole, disk, o, d, rows=None, extra=None):
    """Every plane crossing of the ray's march, in row order, over the rows the march takes: row j is
    taken iff j < max_steps and the swept angle after row j - 1 is below 2 pi; the chain ends with its
    first captured row (that row's crossing is listed: the caller lets the capture win).  The
    restated chain has no escape cutoff; rows beyond an escape are the caller's to cut."""
    if rows is None:
        rows, extra = ol.kerr_chain_st(hole.bh, hole.kerr[0], hole.kerr[1], o, d, 1.0, max_rows=hole.max_steps)
    out = []
    qi, pi = kerr_init(hole, o, d)
    n = len(rows)
    if n > 1:  # the rows the march takes: up to the first whose predecessor swept 2 pi
        done = np.flatnonzero(~(extra[:n - 1, 0] < 2.0 * math.pi))
        if len(done):
            n = int(done[0]) + 1
    z0 = np.concatenate([[qi[2]], rows[:n - 1, 10]])
    z1 = rows[:n, 10]
    for j in np.flatnonzero(((z0 > 0.0) & (z1 <= 0.0)) | ((z0 < 0.0) & (z1 >= 0.0))):
        j = int(j)
        q0, p0 = (qi, pi) if j == 0 else ([float(v) for v in rows[j - 1, 8:11]], [float(v) for v in rows[j - 1, 11:14]])
        q1, p1 = [float(v) for v in rows[j, 8:11]], [float(v) for v in rows[j, 11:14]]
        c = Crossing()
        c.row = j
        c.s = q0[2] / (q0[2] - q1[2])
        c.x = q0[0] + c.s * (q1[0] - q0[0])
        c.y = q0[1] + c.s * (q1[1] - q0[1])
        c.r2 = (c.x * c.x + c.y * c.y) - hole.a2
        c.on = disk.r_in2 <= c.r2 <= disk.r_out2
        c.side = 1.0 if q0[2] > 0.0 else -1.0
        c.captured = bool(rows[j, 7])
        if c.on:
            mt = float(rows[j, 6])
            c.t = c.s * mt
            c.hit_p = np.array([float(rows[j, i]) + float(rows[j, 3 + i]) * c.t for i in range(3)])
            c.w_out = -rows[j, 3:6]
            px = p0[0] + c.s * (p1[0] - p0[0])
            py = p0[1] + c.s * (p1[1] - p0[1])
            c.lz = c.x * py - c.y * px
            c.r = math.sqrt(c.r2)
            c.g = redshift(hole, disk, c.r, c.lz) if disk.redshift else 1.0
            cc = disk.r_in / c.r
            w = (cc * cc) * cc
            if disk.redshift:
                g2 = c.g * c.g
                w = w * (g2 * g2)
            c.w = w
            c.rgb = disk.emission * np.float32(w)
            gs = c.g if c.side > 0 else -c.g
            c.n = np.array([hole.ez[i] * gs for i in range(3)])
        out.append(c)
    return out


def first_on(cr):
    for c in cr:
        if c.on:
            return c
    return None


def disk_record(c):
    r = np.zeros((), rrt.HIT_DTYPE)
    r["status"], r["prim"], r["bsdf"], r["steps"] = DISK, -1, -1, c.row + 1
    r["hit_p"], r["n"], r["w_out"], r["t"] = c.hit_p, c.n, c.w_out, c.t
    return r


def expected_record(hole, disk, o, d, un):
    """The disk-aware closest-hit record of a ray from its checked disk-less record `un` (no exit mode):
    (record, kind) with kind in 'none' (no annulus crossing within the march), 'before' (a hit or
    capture on an earlier row stays), 'capture' (same row: the capture wins), 'prim' (same row: the
    primitive's t <= t_disk), 'disk_contest' (same row: the disk is nearer), 'disk'."""
    st, steps = int(un["status"]), int(un["steps"])
    c = first_on(crossings(hole, disk, o, d))
    if c is None:
        return un.copy(), "none"
    if st in (HIT, CAPTURED):
        if steps - 1 < c.row:
            return un.copy(), "before"
        if steps - 1 == c.row:
            if st == CAPTURED:
                return un.copy(), "capture"
            if float(un["t"]) <= c.t:
                return un.copy(), "prim"
            return disk_record(c), "disk_contest"
        return disk_record(c), "disk"
    # a MISS: an escape at row steps - 1 (that step makes no chord) or a budget end after `steps` rows
    last = steps - 1 if xc.kerr_budget_end(hole.bh, hole.kerr, o, d, steps, hole.max_steps) else steps - 2
    if c.row > last:
        return un.copy(), "none"
    return disk_record(c), "disk"


def expected_records(hole, disk, o, d, un):
    """expected_record for a ray set: (records [n], kinds [n])."""
    out = un.copy()
    kinds = []
    for i in range(len(o)):
        out[i], k = expected_record(hole, disk, o[i], d[i], un[i])
        kinds.append(k)
    return out, kinds


def as_any(rec):
    """The shadow query's records: status and steps (and an ESCAPED record's w_out) alone."""
    return xc.as_any(rec)


# ------------------------------------------------------------------ the CPU-only disk-less record
def cpu_diskless(orc, prims, hole, o, d, answer):
    """(status, steps, t) of the disk-less Kerr march of one ray from the restatement alone, for the
    counts the ray sets must show: a hit's row is the first chord the restated hit point lies on
    (to 1e-9), its t the distance along it; a capture ends the chain; otherwise MISS with steps = -1
    (the escape row is not needed: the disk lies inside the escape radius)."""
    rows, extra = ol.kerr_chain_st(hole.bh, hole.kerr[0], hole.kerr[1], o, d, 1.0, max_rows=hole.max_steps)
    hit, hp = answer[0], answer[1]
    if hit:
        for j in range(len(rows)):
            v = hp - rows[j, 0:3]
            t = float(v @ rows[j, 3:6])
            if -1e-9 <= t <= rows[j, 6] + 1e-9 and np.linalg.norm(v - t * rows[j, 3:6]) < 1e-9:
                return HIT, j + 1, t, rows, extra
        raise AssertionError("the restated hit point lies on no chord of the restated chain")
    if rows[-1, 7]:
        return CAPTURED, len(rows), 0.0, rows, extra
    return MISS, -1, 0.0, rows, extra


def cpu_counts(orc, prims, hole, disk, o, d, answers):
    """By the CPU rule alone: {'disk': DISK records, 'through': rays that cross the plane inside r_in or
    outside r_out and go on (a crossing off the annulus on a row the march lives to finish),
    'contest': rows holding an annulus crossing and the ray's primitive hit}."""
    n = {"disk": 0, "through": 0, "contest": 0}
    for i in range(len(o)):
        st, steps, t, rows, extra = cpu_diskless(orc, prims, hole, o[i], d[i], answers[i])
        end = steps - 1 if st != MISS else len(rows)  # the row that ends the disk-less march
        cr = [c for c in crossings(hole, disk, o[i], d[i], rows, extra) if c.row <= end]
        c = first_on(cr)
        stop = c.row if c is not None else end
        if any((not x.on) and x.row < stop for x in cr):
            n["through"] += 1
        if c is None:
            continue
        if c.row < end or st == MISS:
            n["disk"] += 1
        elif st == HIT:
            n["contest"] += 1
            if t > c.t:
                n["disk"] += 1
    return n


# ------------------------------------------------------------------ ray sets
def annulus_rays(hole, r_lo, r_hi, n=512, seed=11, dist=(0.15, 0.6)):
    """Rays aimed at points of the equatorial plane with r in [r_lo, r_hi] M (uniform in r and
    azimuth), from origins `dist` scene units away in directions within 70 degrees of the plane's
    normal, either side."""
    g = np.random.default_rng(seed)
    ex, ey, ez, c = (np.array(v) for v in (hole.ex, hole.ey, hole.ez, hole.c))
    r = hole.m * (r_lo + (r_hi - r_lo) * g.random(n))
    ph = 2 * np.pi * g.random(n)
    tgt = c + (r * np.cos(ph))[:, None] * ex + (r * np.sin(ph))[:, None] * ey
    th = np.radians(70.0) * g.random(n)
    az = 2 * np.pi * g.random(n)
    side = np.where(g.random(n) < 0.5, -1.0, 1.0)
    u = (np.sin(th) * np.cos(az))[:, None] * ex + (np.sin(th) * np.sin(az))[:, None] * ey + (side * np.cos(th))[:, None] * ez
    o = tgt + (dist[0] + (dist[1] - dist[0]) * g.random(n))[:, None] * u
    return o, tc.unit(tgt - o)


# ------------------------------------------------------------------ what tests/test_gpu_disk.py traces
# CBspheres with the default hole as Kerr; the disk ISCO..16 M, and ISCO..30 M for the same-row contests
KERRS = {"a0.9": (0.9, (0.3, 1.0, -0.2)), "a0": (0.0, (0.0, 1.0, 0.0))}
R_OUT, R_OUT_WIDE = 16.0, 30.0
GPU_SETS = ("interior", "annulus", "camera")
CAMERA_CASE = "spheres_96x72_s1"


def camera_rays(case, xs, ys):
    """The pixel-centre camera rays of pixels (xs, ys) of a golden case's frame (ro_camera_ray)."""
    import ctypes as C
    cam = ol.load_camera(case.camera_path)
    cols = np.array(cam.c2w, np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(cam.pos, np.float64)
    o, d = np.zeros((len(xs), 3)), np.zeros((len(xs), 3))
    mn, mx = C.c_double(), C.c_double()
    for i, (x, y) in enumerate(zip(xs, ys)):
        ol.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, (x + 0.5) / case.frame_w,
                               (y + 0.5) / case.frame_h, o[i], d[i], C.byref(mn), C.byref(mx))
    return o, d


def gpu_rays(name, hole, stride=3):
    """The rays of a GPU ray set: two 512-ray sets, and the 96 x 72 camera frame (every stride-th pixel
    both ways: the CPU counts take stride 3, the GPU test the whole frame)."""
    if name == "interior":
        return tc.ray_sets()["interior"]
    if name == "annulus":
        return annulus_rays(hole, 1.0, 34.0)
    from golden_cases import Case
    c = Case(CAMERA_CASE)
    xs, ys = (a.ravel() for a in np.meshgrid(np.arange(0, c.frame_w, stride), np.arange(0, c.frame_h, stride)))
    return camera_rays(c, xs, ys)
