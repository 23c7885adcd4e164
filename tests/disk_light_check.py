"""The CPU rule of the disk light (RRT_DISK_LIGHT, rrt_disk_sample), restated from
DESIGN.md §14 in Python floats: one correctly rounded IEEE operation at a time, no contraction, in the
order fixed there.  sin and cos are math.sin and math.cos, the host C library's; the device evaluates
rrt_glibm.h's restatements of them, which return the library's bits under the parity precondition of
tests/test_glibm.py -- the tests that compare bits skip loudly where it does not hold.

disk_sample is `sample`.  disk_direct is split in two, because the shadow rays of many pixels are
traced and checked together: `pixel_samples` gives a pixel's light samples from its camera record and
its keyed draws (the shadow ray of each sample that gets one), `pixel_term` folds the radiances those
rays return into the pixel's term D.  Builds on tests/disk_check.py (Hole, Disk, crossings) and
tests/blackbody_check.py (the blackbody colour).
"""
import ctypes as C
import math

import numpy as np

import blackbody_check as bb
import disk_check as dc
import oracle_lib as ol
import rrt

PI = 3.14159265358979323   # rrt_device.h PI_D
EPS = 0.00000000001        # rrt_device.h EPS_D
RAND_MAX = 2147483647.0


def parity():
    """None where math.sin / math.cos are the functions rrt_glibm.h restates, else why not."""
    from test_glibm import precondition
    return precondition()


def div(a, b):
    """IEEE a / b, division by zero included."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def f32(x):
    with np.errstate(all="ignore"):
        return np.float32(x)


class Light:
    """The constants rrt_host.cpp fill_disk_params adds for the disk light, from a checker disk
    (dc.Disk or bb.Disk): the annulus in the Kerr-Schild plane, where x^2 + y^2 = r^2 + a^2."""

    def __init__(self, hole, disk):
        self.hole, self.disk = hole, disk
        self.rho_in2 = disk.r_in2 + hole.a2
        self.rho_span = disk.r_out2 - disk.r_in2
        self.area = PI * self.rho_span


def world(hole, x, y, z):
    """rrt_device.h kerr_world."""
    return [hole.c[i] + ((hole.ex[i] * x + hole.ey[i] * y) + hole.ez[i] * z) for i in range(3)]


def point(light, u, v):
    """Steps 1-3: the local (x, y) of the sampled point."""
    rho = math.sqrt(light.rho_in2 + u * light.rho_span)
    phi = (2.0 * PI) * v
    return rho * math.cos(phi), rho * math.sin(phi)


def sample(light, p, u, v):
    """disk_sample: (ok, wi [3], pdf float32)."""
    h = light.hole
    x, y = point(light, u, v)
    P = world(h, x, y, 0.0)
    dv = [P[i] - float(p[i]) for i in range(3)]
    d2 = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]
    inv = div(1.0, math.sqrt(d2))
    wi = [dv[0] * inv, dv[1] * inv, dv[2] * inv]
    c = abs((wi[0] * h.ez[0] + wi[1] * h.ez[1]) + wi[2] * h.ez[2])
    pdf = f32(div(d2, light.area * c))
    return bool(np.isfinite(pdf) and pdf > 0.0), wi, pdf


def sample_many(light, p, uv):
    """rrt_disk_sample: (wi float64 [n, 3], pdf float32 [n]), an invalid sample's pdf 0."""
    wi, pdf = np.zeros((len(p), 3)), np.zeros(len(p), np.float32)
    for i in range(len(p)):
        ok, w, f = sample(light, p[i], float(uv[i][0]), float(uv[i][1]))
        wi[i] = w
        pdf[i] = f if ok else 0.0
    return wi, pdf


# ------------------------------------------------------------------ the scene's BSDFs
class BsdfDesc(C.Structure):  # rrt_bsdf_desc
    _fields_ = [("type", C.c_uint32), ("params", C.c_float * 14)]


def bsdfs_of(scene_file):
    """[(type, params float32 [14])] of a SceneFile."""
    d = rrt.SceneDesc.from_address(scene_file.desc())
    arr = C.cast(d.bsdfs, C.POINTER(BsdfDesc))
    return [(int(arr[i].type), np.array(arr[i].params, np.float32)) for i in range(d.n_bsdfs)]


def diffuse_f(params):
    """bsdf_f of a diffuse BSDF: albedo / (float)PI_D, whatever the directions."""
    return params[:3].astype(np.float32) / np.float32(PI)


def n_listed_draws(scene_file, ns_area_light, env=False):
    """The draws direct_importance takes at one shading point of a scene with area and point lights:
    two per area-light sample, none for a point light; env: the environment light's samples too, two
    draws each."""
    d = rrt.SceneDesc.from_address(scene_file.desc())
    return sum(0 if d.lights[i].is_delta else 2 * ns_area_light for i in range(d.n_lights)) + (2 * ns_area_light if env else 0)


# ------------------------------------------------------------------ disk_direct
def to_local_z(n, wi):
    """w_in.z of disk_direct: to_local(coord_space(n), wi).z (the restated make_coord_space)."""
    o2w, a, b = np.zeros(9), np.zeros(3), np.zeros(3)
    ol.lib().ro_coord_space(np.ascontiguousarray(n, np.float64), np.ascontiguousarray(wi, np.float64), o2w, a, b)
    return float(a[2])


class Sample:
    """One light sample of a pixel: ok (disk_sample's), wi, pdf, cos (w_in.z), shadow (a shadow ray is
    traced: ok and cos >= 0), o (its origin hit_p + EPS wi)."""


def pixel_samples(light, hit_p, n, key, first_draw, ns_area_light):
    """The ns_area_light samples disk_direct takes at the hit (hit_p, n) of the pixel with RNG key `key`,
    whose draw counter stands at first_draw when the disk's term begins (every listed light's draws are
    behind it).  g.grid(u, v) draws v first."""
    out = []
    for i in range(ns_area_light):
        v = ol.lib().ro_keyed_rand(key, first_draw + 2 * i) / RAND_MAX
        u = ol.lib().ro_keyed_rand(key, first_draw + 2 * i + 1) / RAND_MAX
        s = Sample()
        s.u, s.v = u, v
        s.ok, s.wi, s.pdf = sample(light, hit_p, u, v)
        s.cos = to_local_z(n, s.wi) if s.ok else math.nan
        s.shadow = s.ok and not s.cos < 0
        s.o = [float(hit_p[k]) + EPS * s.wi[k] for k in range(3)] if s.shadow else None
        out.append(s)
    return out


def pixel_term(samples, rgbs, f):
    """D = L / (float)ns_area_light, L the sum over the samples whose shadow ray ended on the disk of
    ((rgb * f) * (float)cos) / pdf in float32; rgbs[i]: float32 [3], or None where sample i's ray did not
    (or it has none); f: bsdf_f float32 [3]."""
    L = np.zeros(3, np.float32)
    for s, rgb in zip(samples, rgbs):
        if rgb is None:
            continue
        assert s.shadow
        with np.errstate(all="ignore"):
            L = L + ((np.asarray(rgb, np.float32) * f) * np.float32(s.cos)) / s.pdf
    return L / np.float32(len(samples))


# ------------------------------------------------------------------ what tests/test_gpu_disk_light.py renders
# CBspheres through the wide camera (the whole room), the default hole as Kerr (dc.KERRS), the disk
# ISCO..16 M; 96 x 72, ns_aa = 1, depth 1, ns_area_light = 4; every STRIDE-th pixel both ways is checked
WIDE_CASE = "cfg1_spheres_480x360_s8"
W, H, NS_AREA_LIGHT, STRIDE = 96, 72, 4, 3
DIFFUSE = 0  # RRT_BSDF_DIFFUSE


def frame_pixels(stride=STRIDE):
    xs, ys = (a.ravel() for a in np.meshgrid(np.arange(0, W, stride), np.arange(0, H, stride)))
    return xs, ys


def camera_rays(camera_path, xs, ys):
    """The pixel-centre camera rays of pixels (xs, ys) of the W x H frame of a camera file (ro_camera_ray)."""
    cam = ol.load_camera(camera_path)
    cols = np.array(cam.c2w, np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(cam.pos, np.float64)
    o, d = np.zeros((len(xs), 3)), np.zeros((len(xs), 3))
    mn, mx = C.c_double(), C.c_double()
    for i, (x, y) in enumerate(zip(xs, ys)):
        ol.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, (x + 0.5) / W, (y + 0.5) / H, o[i], d[i],
                               C.byref(mn), C.byref(mx))
    return o, d


def checkable(bsdfs, bsdf, n):
    """A hit the pixel test checks: non-emissive and non-delta (here: diffuse) with an axis-aligned
    shading normal (the floor and the walls: two components within 1e-6 of 0 -- the scene file's normals
    are floats of a rotated room, off the axes by 1.5e-7)."""
    a = np.abs(np.asarray(n, np.float64))
    return bsdf >= 0 and bsdfs[bsdf][0] == DIFFUSE and int((a <= 1e-6 * a.max()).sum()) == 2


def cpu_outcome(hole, disk, o, d, answer):
    """By the CPU rule alone, how the disk-aware closest-hit march of the ray ends: 'disk', 'prim',
    'capture' or 'none' (dc.cpu_counts' case analysis for one ray)."""
    st, steps, t, rows, extra = dc.cpu_diskless(None, None, hole, o, d, answer)
    end = steps - 1 if st != dc.MISS else len(rows)
    c = dc.first_on([c for c in dc.crossings(hole, disk, o, d, rows, extra) if c.row <= end])
    if c is not None and (c.row < end or st == dc.MISS or (st == dc.HIT and t > c.t)):
        return "disk"
    return {dc.HIT: "prim", dc.CAPTURED: "capture", dc.MISS: "none"}[st]


def crossing_rgb(disk, c):
    """The radiance of a checked crossing on the annulus under the disk's colour rule."""
    return bb.crossing_rgb(disk, c) if isinstance(disk, bb.Disk) else c.rgb


def shadow_crossing(hole, disk, o, d, un):
    """Where the closest-hit march of disk_direct's shadow ray (o, d) ends, from the ray's checked
    disk-less record `un`: (the crossing, or None where the expected record is no DISK record, kind,
    the expected record's status) -- dc.expected_record's kinds.  crossing_rgb of the crossing is the
    radiance the sample takes."""
    rec, kind = dc.expected_record(hole, disk, o, d, un)
    if int(rec["status"]) != dc.DISK:
        return None, kind, int(rec["status"])
    return dc.first_on(dc.crossings(hole, disk, o, d)), kind, dc.DISK
