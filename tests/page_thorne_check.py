"""The CPU rule of the Page-Thorne temperature profile of the blackbody disk
(RRT_DISK_PROFILE_PAGE_THORNE), restated from DESIGN.md §15 in Python floats: one
correctly rounded IEEE operation at a time, no contraction, in the order fixed there.  log, acos and cos
are math.log, math.acos and math.cos, the host C library's; the library evaluates rrt_glibm.h's
restatements of them (acos and cos on the host only, log on the host and the device), which return the
library's bits under the parity precondition of tests/test_glibm.py -- the tests that compare bits skip
loudly where it does not hold.

Builds on tests/blackbody_check.py: the Planck part of the colour (`planck`) is blackbody_check.rgb's,
restated here because blackbody_check.temperature falls back to the power profile for a profile it
does not know.
"""
import math

import numpy as np

import blackbody_check as bb
import disk_check as dc

PI = 3.14159265358979323   # rrt_device.h PI_D
PAGE_THORNE = 3
PROFILES = dict(bb.PROFILES, **{"page-thorne": PAGE_THORNE})
ROUNDS = 200               # of the peak search
BLACK = bb.BLACK


def parity():
    """None where math.log / acos / cos / exp are the functions rrt_glibm.h restates, else why not."""
    return bb.parity()


def div(a, b):
    """IEEE a / b, division by zero included."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def log(x):
    """The library's log: -inf at 0, NaN below it."""
    if x != x or x < 0.0:
        return math.nan
    if x == 0.0:
        return -math.inf
    return math.log(x)


def sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


class Disk(bb.Disk):
    """bb.Disk plus the Page-Thorne constants of rrt_host.cpp fill_disk_params (rrt_blackbody.cpp
    rrt_pt_constants): s = a / M, x0 (the device's x of r_in), ca = 1.5 s, a2 = 2 s, the roots x[3] of
    x^3 - 3 x + 2 s, d[i] = x0 - x[i], their coefficients c[3] and norm = 1 / S(x_peak)."""

    def __init__(self, hole, r_in, r_out, emission, redshift=True, temperature=6000.0, profile=PAGE_THORNE):
        super().__init__(hole, r_in, r_out, emission, redshift, temperature, PROFILES.get(profile, profile))
        assert self.profile == PAGE_THORNE
        s = hole.a / hole.m if hole.m > 0.0 else 0.0
        self.s = s
        self.x0 = math.sqrt(self.r_in) / self.sqrt_m
        self.ca = 1.5 * s
        self.a2 = 2.0 * s
        t = math.acos(s) / 3.0
        p3 = PI / 3.0
        self.x = [2.0 * math.cos(t - p3), 2.0 * math.cos(t + p3), -(2.0 * math.cos(t))]
        self.d = [self.x0 - xi for xi in self.x]
        self.c = []
        for i in range(3):
            xi, xj, xk = self.x[i], self.x[(i + 1) % 3], self.x[(i + 2) % 3]
            e = xi - s
            c = div(3.0 * (e * e), xi * ((xi - xj) * (xi - xk)))
            self.c.append(c if math.isfinite(c) else 0.0)
        self.norm = 1.0
        self.x_peak = peak(self)
        self.norm = div(1.0, shape(self, self.x_peak))


def shape(disk, x):
    """S(x) in the device's operation order (steps 2-6 of §15 without the norm)."""
    B = (x - disk.x0) - disk.ca * log(div(x, disk.x0))
    for i in range(3):
        B = B - disk.c[i] * log(div(x - disk.x[i], disk.d[i]))
    x2 = x * x
    den = (x2 * x2) * (((x2 * x) - 3.0 * x) + disk.a2)
    return div(B, den)


def shape_np(disk, x):
    """shape on an array of x, with numpy's log: for the luminosity integral's 2e5 radii (agrees with
    shape to 1e-12, tests/test_page_thorne_rule.py)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        B = (x - disk.x0) - disk.ca * np.log(x / disk.x0)
        for i in range(3):
            B = B - disk.c[i] * np.log((x - disk.x[i]) / disk.d[i])
        x2 = x * x
        return B / ((x2 * x2) * (((x2 * x) - 3.0 * x) + disk.a2))


def peak(disk):
    """The fixed ternary search for the x of S's maximum: 200 rounds from [x0, 2 x0]."""
    lo, hi = disk.x0, 2.0 * disk.x0
    for _ in range(ROUNDS):
        m1 = lo + (hi - lo) / 3.0
        m2 = hi - (hi - lo) / 3.0
        if shape(disk, m1) < shape(disk, m2):
            lo = m1
        else:
            hi = m2
    return 0.5 * (lo + hi)


def x_of(disk, r):
    """Step 1: x = sqrt(r) / sqrt(M), r in scene units."""
    return div(sqrt(r), disk.sqrt_m)


def q_of(disk, r):
    """q = S(x) norm at radius r (scene units): 1 at the peak, 0 at r_in; no disk below r_in (x < x0 or
    NaN: None, black -- the device returns before it forms B)."""
    x = x_of(disk, r)
    if not x >= disk.x0:
        return None
    return shape(disk, x) * disk.norm


def r_peak(disk):
    """The peak's radius in scene units (x^2 M; the checker's own, to place a sample at the peak)."""
    return (disk.x_peak * disk.x_peak) * (disk.sqrt_m * disk.sqrt_m)


def planck(disk, q, g):
    """§13 from `if (!(q > 0)) black` onward: float32 [3]."""
    if q is None or not q > 0.0:
        return BLACK.copy()
    t = disk.temperature * math.sqrt(math.sqrt(q))
    t_obs = (g if disk.redshift else 1.0) * t
    if not (t_obs > 0.0 and math.isfinite(t_obs)):
        return BLACK.copy()
    out = np.zeros(3, np.float32)
    for k in range(3):
        den = bb.exp(div(disk.K[k], t_obs)) - 1.0
        ratio = div(disk.N[k], den)
        if not math.isfinite(ratio):
            ratio = 0.0
        out[k] = disk.emission[k] * np.float32(ratio)
    return out


def rgb(disk, r, g):
    """disk_rgb<true, true>: float32 [3] at radius r (scene units) seen at redshift g."""
    return planck(disk, q_of(disk, r), g)


def any_rgb(disk, r, g):
    return rgb(disk, r, g) if isinstance(disk, Disk) else bb.any_rgb(disk, r, g)


def of(hole, got):
    """The checker's disk of a Renderer.get_disk() dict: a Page-Thorne Disk, else blackbody_check.of's."""
    if got.get("profile") == "page-thorne":
        return Disk(hole, got["r_in"], got["r_out"], got["emission"], got["redshift"], got["temperature"])
    return bb.of(hole, got)


def eval_rgb(hole, disk, r_m, g):
    """rrt_disk_eval: float32 [n, 3] at Boyer-Lindquist radii r_m (in M) and redshifts g."""
    with np.errstate(all="ignore"):
        return np.array([any_rgb(disk, float(r) * hole.m, float(x)) for r, x in zip(r_m, g)], np.float32).reshape(-1, 3)


def crossing_rgb(disk, c):
    """The colour of a checked crossing on the annulus (dc.Crossing: r2, g) under the disk's rule."""
    if isinstance(disk, Disk):
        return rgb(disk, math.sqrt(c.r2), c.g)
    return bb.crossing_rgb(disk, c) if isinstance(disk, bb.Disk) else c.rgb


# ------------------------------------------------------------------ the physics the rule is pinned by
def e_dagger(s, r):
    """The specific energy of the prograde circular geodesic at r (in M): Page & Thorne's E-dagger."""
    x = np.sqrt(r)
    return (x ** 3 - 2.0 * x + s) / (x ** 1.5 * np.sqrt(x ** 3 - 3.0 * x + 2.0 * s))


def efficiency(disk, n=200000, r_max=1e6):
    """The luminosity integral of 1.5 r S(sqrt r) E-dagger(r) dr from r_in to r_max (in M): the
    trapezium rule on n log-spaced radii.  Equals 1 - E-dagger(r_in) for the exact flux."""
    r = np.geomspace(disk.r_in_m, r_max, n)
    f = 1.5 * r * shape_np(disk, np.sqrt(r)) * e_dagger(disk.s, r)
    return float(np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(r)))
