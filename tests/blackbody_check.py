"""The CPU rule of the blackbody accretion disk (RRT_DISK_BLACKBODY, rrt_disk_eval),
restated from DESIGN.md §13 in Python floats: one correctly rounded IEEE operation at a time, no
contraction, in the order fixed there.  exp is math.exp, the host C library's; the device evaluates
rrt_glibm.h's restatement of it, which returns the library's bits under the parity precondition of
tests/test_glibm.py (the pinned libm build on an FMA host) -- the tests that compare bits skip loudly
where it does not hold.

Builds on tests/disk_check.py: a Disk carries the plain disk's device constants, a Crossing the radius
(r2) and the redshift (g) of a ray's crossing.
"""
import math

import numpy as np

import disk_check as dc

HC_K = 14387768.77               # hc / k in nm K
LAMBDA = (610.0, 550.0, 465.0)   # the channels' wavelengths in nm
F_NORM = 823543.0 / 46656.0      # 1 / max of c^3 (1 - sqrt c), reached at c = 36 / 49
T_MIN, T_MAX = 1000.0, 1e6
POWER, ZERO_TORQUE = 0, 1
PROFILES = {"power": POWER, "zero-torque": ZERO_TORQUE}
BLACK = np.zeros(3, np.float32)


def parity():
    """None where math.exp is the exp rrt_glibm.h restates, else why not (tests/test_glibm.py)."""
    from test_glibm import precondition
    return precondition()


def exp(x):
    try:
        return math.exp(x)
    except OverflowError:  # the library returns +inf there
        return math.inf


class Disk(dc.Disk):
    """dc.Disk plus the blackbody constants of rrt_host.cpp fill_disk_params: temperature as the
    descriptor's float holds it, the profile, K_c = HC_K / lambda_c and N_c = exp(K_c / temperature) - 1."""

    def __init__(self, hole, r_in, r_out, emission, redshift=True, temperature=6000.0, profile=POWER):
        super().__init__(hole, r_in, r_out, emission, redshift)
        self.temperature = float(np.float32(temperature))
        self.profile = PROFILES.get(profile, profile)
        self.K = [HC_K / lam for lam in LAMBDA]
        self.N = [exp(k / self.temperature) - 1.0 for k in self.K]


def of(hole, got):
    """The checker's disk of a Renderer.get_disk() dict: a blackbody Disk, or dc.Disk for a plain one."""
    if "temperature" in got:
        return Disk(hole, got["r_in"], got["r_out"], got["emission"], got["redshift"], got["temperature"], got["profile"])
    return dc.Disk(hole, got["r_in"], got["r_out"], got["emission"], got["redshift"])


def temperature(disk, r):
    """(q, T) at radius r (scene units): T = temperature x q^(1/4); q <= 0 or NaN: the gas is black (T None)."""
    c = disk.r_in / r if r != 0.0 else math.copysign(math.inf, disk.r_in) * math.copysign(1.0, r)
    c3 = (c * c) * c
    q = c3
    if disk.profile == ZERO_TORQUE:
        q = (c3 * (1.0 - (math.sqrt(c) if c >= 0.0 else math.nan))) * F_NORM
    if not q > 0.0:
        return q, None
    return q, disk.temperature * math.sqrt(math.sqrt(q))


def rgb(disk, r, g):
    """disk_rgb<true>: float32 [3] at radius r (scene units) seen at redshift g."""
    _, t = temperature(disk, r)
    if t is None:
        return BLACK.copy()
    t_obs = (g if disk.redshift else 1.0) * t
    if not (t_obs > 0.0 and math.isfinite(t_obs)):
        return BLACK.copy()
    out = np.zeros(3, np.float32)
    for k in range(3):
        den = exp(disk.K[k] / t_obs) - 1.0
        ratio = disk.N[k] / den if den != 0.0 else math.inf
        if not math.isfinite(ratio):
            ratio = 0.0
        out[k] = disk.emission[k] * np.float32(ratio)
    return out


def plain_rgb(disk, r, g):
    """disk_rgb<false>, as disk_check.crossings has it: emission x (float)(c^3 g^4)."""
    c = disk.r_in / r
    w = (c * c) * c
    if disk.redshift:
        g2 = g * g
        w = w * (g2 * g2)
    return disk.emission * np.float32(w)


def any_rgb(disk, r, g):
    return rgb(disk, r, g) if isinstance(disk, Disk) else plain_rgb(disk, r, g)


def eval_rgb(hole, disk, r_m, g):
    """rrt_disk_eval: float32 [n, 3] at Boyer-Lindquist radii r_m (in M) and redshifts g."""
    with np.errstate(all="ignore"):
        return np.array([any_rgb(disk, float(r) * hole.m, float(x)) for r, x in zip(r_m, g)], np.float32).reshape(-1, 3)


def crossing_rgb(disk, c):
    """The colour of a checked crossing on the annulus (dc.Crossing: r2, g)."""
    return rgb(disk, math.sqrt(c.r2), c.g)


def tint(t):
    """rrt_blackbody_tint to double precision: W_c (exp(K_G / T) - 1) / (exp(K_c / T) - 1), W_c = (550 / lambda_c)^5."""
    n = [exp(HC_K / lam / t) - 1.0 for lam in LAMBDA]
    return [(550.0 / lam) ** 5 * n[1] / n[k] for k, lam in enumerate(LAMBDA)]
