"""The Page-Thorne temperature profile of the blackbody disk (RRT_DISK_PROFILE_PAGE_THORNE)
on the CPU: the enum, the names and the descriptor's validation on a host-only context, and the rule of
tests/page_thorne_check.py pinned by physics -- the black inner edge, the peak's position, the
luminosity integral returning the textbook efficiencies, the Newtonian limit -- before
tests/test_gpu_page_thorne.py compares the GPU with it bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import blackbody_check as bb
import disk_check as dc
import page_thorne_check as pt
import rrt
import trace_check as tc
from test_blackbody_rule import EM, desc

AXIS = (0.0, 1.0, 0.0)
# (spin, r_in in M or None for the ISCO): the cases of the efficiency and Newtonian pins
CASES = [(0.0, None), (0.5, None), (0.9, None), (0.0, 20.0)]


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


def disk_of(spin, r_in=None, r_out=16.0, redshift=True, temperature=6000.0, axis=AXIS):
    hole = dc.Hole(tc.DEFAULT_BH, (spin, axis))
    r_in = dc.isco(spin) if r_in is None else r_in
    return hole, pt.Disk(hole, r_in, max(r_out, 2.0 * r_in), EM, redshift, temperature)


# ------------------------------------------------------------------ the enum, the names, validation
def test_enum_and_names():
    assert rrt.RRT_DISK_PROFILE_PAGE_THORNE == 3 and pt.PAGE_THORNE == 3
    assert rrt.DISK_PROFILES == {"power": 0, "zero-torque": 1, "page-thorne": 3}
    assert pt.PROFILES == rrt.DISK_PROFILES
    assert C.sizeof(rrt.DiskDesc) == 48 and rrt.lib().rrt_abi_version() == 5


def test_set_get_round_trip(host):
    host.set_disk(7.0, 16.0, emission=EM, temperature=6000.0, profile="page-thorne")
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": EM, "redshift": True,
                               "temperature": 6000.0, "profile": "page-thorne"}
    d = rrt.DiskDesc()
    assert rrt.lib().rrt_get_disk(host.h, C.byref(d)) == 1
    assert d.flags == rrt.RRT_DISK_BLACKBODY and d.profile == 3 and bytes(d)[40:48] == bytes(8)
    host.set_disk(7.0, 16.0, emission=EM, temperature=4500.0, profile="page-thorne", redshift=False, light=True)
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": EM, "redshift": False, "temperature": 4500.0,
                               "profile": "page-thorne", "light": True}
    host.set_disk(7.0, 16.0, emission=EM, temperature=6000.0, profile=rrt.RRT_DISK_PROFILE_PAGE_THORNE)
    assert host.get_disk()["profile"] == "page-thorne"
    host.set_disk(0.0, 16.0, temperature=6000.0, profile="page-thorne")
    host.set_black_hole(spin=0.9)
    assert abs(host.get_disk()["r_in"] - dc.isco(0.9)) < 1e-14 and host.get_disk()["emission"] == rrt.blackbody_tint(6000.0)


@pytest.mark.parametrize("profile", [2, 4, 5, 0xFFFFFFFF])
def test_unassigned_profiles_stay_invalid(host, profile):
    host.set_disk(7.0, 20.0)
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(profile=profile))) == rrt.RRT_E_INVALID
    assert host.get_disk()["r_out"] == 20.0  # still in force
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(profile=3))) == rrt.RRT_OK


def test_without_the_blackbody_flag_the_profile_is_not_read(host):
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(flags=0, profile=3))) == rrt.RRT_OK
    assert set(host.get_disk()) == {"r_in", "r_out", "emission", "redshift"}
    d = rrt.DiskDesc()
    assert rrt.lib().rrt_get_disk(host.h, C.byref(d)) == 1 and d.profile == 0


def test_launch_time_errors_need_no_device(host):
    """The errors of §12 in their order: the Schwarzschild kind, then the device; an r_in below the ISCO."""
    r, g = np.array([8.0]), np.array([1.0])
    host.set_disk(0.0, 16.0, temperature=6000.0, profile="page-thorne")
    with pytest.raises(rrt.RRTError) as e:
        host.disk_eval(r, g)
    assert e.value.code == rrt.RRT_E_INVALID and "spin 0" in str(e.value)
    host.set_black_hole(spin=0.5)
    with pytest.raises(rrt.RRTError) as e:
        host.disk_eval(r, g)
    assert e.value.code == rrt.RRT_E_NO_DEVICE
    host.set_disk(4.0, 16.0, temperature=6000.0, profile="page-thorne")
    with pytest.raises(rrt.RRTError) as e:
        host.disk_eval(r, g)
    assert e.value.code == rrt.RRT_E_INVALID and "ISCO" in str(e.value)


# ------------------------------------------------------------------ the constants
@pytest.mark.parametrize("spin", [0.0, 0.3, 0.5, 0.9, 0.998])
def test_roots_and_coefficients(spin):
    """x_i are the roots of x^3 - 3 x + 2 s in the order x1 > x2 >= 0 > x3, all below x0; the C_i are the
    partial fractions of 3 (x - s)^2 / (x (x^3 - 3 x + 2 s)) at them, whose residue at x = 0 is 1.5 s."""
    hole, d = disk_of(spin)
    s = d.s
    assert s == spin or abs(s - spin) < 1e-15
    for xi in d.x:
        assert abs(xi ** 3 - 3.0 * xi + 2.0 * s) < 1e-14
    assert d.x[0] > d.x[1] > -1e-15 and d.x[2] < 0.0 and d.x0 > d.x[0]
    assert d.ca == 1.5 * s and d.a2 == 2.0 * s and all(math.isfinite(c) for c in d.c)
    for x in (0.37, 2.9, 11.0):
        whole = 3.0 * (x - s) ** 2 / (x * (x ** 3 - 3.0 * x + 2.0 * s))
        parts = 1.5 * s / x + sum(c / (x - xi) for c, xi in zip(d.c, d.x))
        assert abs(whole - parts) < 1e-12 * max(1.0, abs(whole))


def test_the_search_brackets_the_peak():
    """The search's bracket is r_in..4 r_in (x0..2 x0); the peak lies at r / r_in in (1.28, 1.60) for the spins
    and edges of the pins and inside (1.2, 2) up to a/M = 0.998: well inside the bracket.  After 200 rounds
    the bracket has closed and S falls off on both sides of it."""
    for spin, r_in in CASES + [(0.9, 7.0), (0.998, None), (0.5, 40.0)]:
        hole, d = disk_of(spin, r_in)
        ratio = (d.x_peak / d.x0) ** 2
        assert (1.28 < ratio < 1.60) if spin <= 0.9 else (1.2 < ratio < 2.0), (spin, r_in, ratio)
        sp = pt.shape(d, d.x_peak)
        assert sp > 0.0 and d.norm == 1.0 / sp
        assert pt.shape(d, d.x_peak * 0.999) < sp and pt.shape(d, d.x_peak * 1.001) < sp
        assert abs(pt.q_of(d, pt.r_peak(d)) - 1.0) < 1e-12


# ------------------------------------------------------------------ the physics pins
@pytest.mark.parametrize("spin,r_in", CASES + [(0.9, 7.0)])
def test_pin_inner_edge_is_black(spin, r_in):
    """S(x0) == 0.0 exactly (x / x0 == 1 and (x - x_i) / (x0 - x_i) == 1: every log is 0), at the x the
    device forms from r_in M too; rgb at r_in is black."""
    hole, d = disk_of(spin, r_in)
    assert pt.shape(d, d.x0) == 0.0 and not math.copysign(1.0, pt.shape(d, d.x0)) < 0
    assert pt.x_of(d, d.r_in) == d.x0
    assert pt.q_of(d, d.r_in) == 0.0
    assert not pt.rgb(d, d.r_in, 1.0).any()
    # the gas outside glows; at an ISCO edge B grows as (x - x0)^2 (the integrand vanishes there too), so
    # within 1e-8 of the edge q is rounding noise of order 1e-15, either sign: black either way (T_obs ~ 1 K)
    assert pt.q_of(d, d.r_in * 1.001) > 1e-6
    assert not pt.rgb(d, d.r_in * (1.0 + 1e-9), 1.0).any()


def test_pin_peak_position_and_colour():
    """a/M = 0 with r_in the ISCO: the flux peaks at r = 9.551 M (Page & Thorne 1974, fig. 1; within 0.01 M),
    and the peak pixel at g = 1 shows `emission` to rtol 1e-6; T rises strictly up to the peak and falls
    strictly beyond it."""
    hole, d = disk_of(0.0)
    assert abs(d.x_peak ** 2 - 9.551) < 0.01
    rp = pt.r_peak(d)
    assert abs(rp / hole.m - 9.551) < 0.01
    assert np.allclose(pt.rgb(d, rp, 1.0), EM, rtol=1e-6, atol=0.0)
    out = [pt.q_of(d, rp * f) for f in np.geomspace(1.0, 8.0, 40)]
    assert all(a > b for a, b in zip(out, out[1:]))
    inner = [pt.q_of(d, d.r_in + (rp - d.r_in) * f) for f in np.linspace(0.02, 1.0, 40)]
    assert all(a < b for a, b in zip(inner, inner[1:]))


def test_vectorised_shape_is_the_scalar_one():
    """The efficiency integral evaluates S with numpy's log on 2e5 radii; it is the checker's S to 1e-12."""
    for spin, r_in in CASES:
        hole, d = disk_of(spin, r_in)
        x = np.geomspace(d.x0 * 1.001, 1e3, 57)
        a, b = pt.shape_np(d, x), np.array([pt.shape(d, float(v)) for v in x])
        assert np.allclose(a, b, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("spin,r_in,textbook", [(0.0, None, 0.05719), (0.5, None, 0.08212), (0.9, None, 0.15575),
                                                (0.0, 20.0, 0.02381)])
def test_pin_efficiency(spin, r_in, textbook):
    """The luminosity of both faces, the integral of 1.5 r S(sqrt r) E-dagger(r) dr from r_in to infinity,
    is the binding energy released down to the edge, 1 - E-dagger(r_in), to relative 1e-3: the trapezium rule
    on 2e5 log-spaced radii out to 1e6 M.  (The tail beyond 1e6 M is 1.5 / r_max = 1.5e-6.)"""
    hole, d = disk_of(spin, r_in)
    want = 1.0 - pt.e_dagger(d.s, d.r_in_m)
    got = pt.efficiency(d, 200000, 1e6)
    print(f"a/M {spin} r_in {d.r_in_m:.4f}: integral {got:.6f}, 1 - E(r_in) {want:.6f}")
    assert abs(want - textbook) < 1e-5
    assert abs(got / want - 1.0) < 1e-3


@pytest.mark.parametrize("spin,r_in", CASES)
def test_pin_newtonian_limit(spin, r_in):
    """Far out the flux is the Newtonian zero-torque one, S -> x^-6 (1 - x0 / x): at r = 1e4 r_in the ratio
    lies in (0.98, 1); the deviation falls as 1 / x (it halves, to 20 %, when r grows fourfold)."""
    hole, d = disk_of(spin, r_in)

    def ratio(x):
        return pt.shape(d, x) * x ** 6 / (1.0 - d.x0 / x)

    x = math.sqrt(1e4) * d.x0
    assert 0.98 < ratio(x) < 1.0, ratio(x)
    assert abs((1.0 - ratio(2.0 * x)) / (1.0 - ratio(x)) - 0.5) < 0.1


# ------------------------------------------------------------------ degenerate inputs, the colour shift
@pytest.mark.parametrize("spin,r_in", [(0.9, None), (0.0, None), (0.0, 7.0), (0.0, 20.0)])
def test_pin_degenerate_inputs_are_black(spin, r_in):
    hole, d = disk_of(spin, r_in)
    r = d.r_in * 2.0
    assert pt.rgb(d, r, 1.0).all()
    for g in (0.0, -0.0, -1.0, math.inf, -math.inf, math.nan):
        out = pt.rgb(d, r, g)
        assert not out.any() and np.isfinite(out).all(), g
    # no disk below r_in: between the photon orbit and an edge at the ISCO the bare formula is positive
    # again (B's integrand changes sign at the ISCO), so the rule cuts there by x < x0
    for f in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999999, 1.0 - 2.0 ** -52):
        out = pt.rgb(d, d.r_in * f, 1.0)
        assert not out.any() and np.isfinite(out).all(), f
    for bad in (-r, math.nan, math.inf, -0.0):
        out = pt.rgb(d, bad, 1.0)
        assert not out.any() and np.isfinite(out).all(), bad
    assert not pt.rgb(d, r, 1e-3).any()  # a tiny T_obs overflows exp: N / inf = 0
    assert np.isfinite(pt.rgb(d, r, 3.0)).all() and pt.rgb(d, r, 3.0).all()


def test_every_intermediate_stays_inside_float_over_the_range():
    for t in (1000.0, 1e6):
        for spin in (0.0, 0.9):
            hole, d = disk_of(spin, temperature=t)
            for r in np.geomspace(d.r_in, 16.0 * hole.m, 9):
                for g in (0.05, 1.0, 3.0):
                    assert np.isfinite(pt.rgb(d, float(r), g)).all(), (t, spin, r, g)


def test_pin_approaching_side_is_bluer():
    """g < 1 lowers B / R and dims every channel, g > 1 raises both; with RRT_DISK_NO_REDSHIFT g is ignored."""
    hole, d = disk_of(0.9)
    _, flat = disk_of(0.9, redshift=False)
    for r in (d.r_in * 1.5, d.r_in * 4.0):
        lo, mid, hi = (pt.rgb(d, r, g).astype(np.float64) for g in (0.7, 1.0, 1.4))
        assert lo[2] / lo[0] < mid[2] / mid[0] < hi[2] / hi[0]
        assert (lo < mid).all() and (mid < hi).all()
        assert all(pt.rgb(flat, r, g).tobytes() == mid.astype(np.float32).tobytes() for g in (0.7, 1.0, 1.4, 0.0, math.nan))


def test_spin_moves_the_profile_and_of_knows_the_name():
    """Same r_in and r_out at a/M = 0 and 0.9: the Page-Thorne q differs, the power profile's does not;
    pt.of builds a Page-Thorne disk for the new name and blackbody_check's for the others."""
    (h0, d0), (h9, d9) = disk_of(0.0, 7.0), disk_of(0.9, 7.0)
    qs0, qs9 = ([pt.q_of(d, f * d.r_in) for f in (1.2, 1.5, 2.0)] for d in (d0, d9))
    assert all(abs(a / b - 1.0) > 1e-3 for a, b in zip(qs0, qs9))
    got = {"r_in": 7.0, "r_out": 16.0, "emission": EM, "redshift": True, "temperature": 6000.0, "profile": "page-thorne"}
    assert isinstance(pt.of(h9, got), pt.Disk) and pt.of(h9, got).norm == d9.norm
    for name in ("power", "zero-torque"):
        other = pt.of(h9, dict(got, profile=name))
        assert type(other) is bb.Disk and other.profile == bb.PROFILES[name]
        for f in (1.2, 2.0):
            assert pt.any_rgb(other, f * other.r_in, 0.9).tobytes() == bb.rgb(bb.of(h0, dict(got, profile=name)), f * other.r_in, 0.9).tobytes()
    assert type(pt.of(h9, {k: got[k] for k in ("r_in", "r_out", "emission", "redshift")})) is dc.Disk
