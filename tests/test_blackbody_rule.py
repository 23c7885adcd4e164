"""The blackbody accretion disk (RRT_DISK_BLACKBODY, rrt_blackbody_tint) on the CPU: the
descriptor's layout and validation on a host-only context, the tint, and the rule of
tests/blackbody_check.py pinned by what it must give before tests/test_gpu_blackbody.py compares the GPU
with it bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import blackbody_check as bb
import disk_check as dc
import rrt
import trace_check as tc

EM = (2.0, 1.0, 0.5)


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


def desc(flags=rrt.RRT_DISK_BLACKBODY, temperature=6000.0, profile=0, r_in=7.0, r_out=16.0):
    d = rrt.DiskDesc()
    d.r_in, d.r_out, d.flags, d.temperature, d.profile = r_in, r_out, flags, temperature, profile
    d.emission[0], d.emission[1], d.emission[2] = EM
    return d


def hole_and_disk(profile, redshift=True, temperature=6000.0):
    hole = dc.Hole(tc.DEFAULT_BH, dc.KERRS["a0.9"])
    return hole, bb.Disk(hole, dc.isco(0.9), 16.0, EM, redshift, temperature, profile)


# ------------------------------------------------------------------ layout and flags
def test_layout_flags_and_exports():
    L = rrt.lib()
    assert C.sizeof(rrt.DiskDesc) == 48
    assert rrt.DiskDesc.temperature.offset == 32 and rrt.DiskDesc.profile.offset == 36
    assert rrt.RRT_DISK_NO_REDSHIFT == 1 and rrt.RRT_DISK_BLACKBODY == 4
    assert (rrt.RRT_DISK_PROFILE_POWER, rrt.RRT_DISK_PROFILE_ZERO_TORQUE) == (0, 1)
    assert L.rrt_abi_version() == 5  # additive: the ABI version stays
    for name in ("rrt_disk_eval", "rrt_blackbody_tint"):
        assert name in rrt.EXPORTS and hasattr(L, name)


@pytest.mark.parametrize("flags", [2, 8, 4 | 2, 4 | 8, 1 | 2])
def test_unassigned_flag_bits_are_invalid(host, flags):
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(flags=flags))) == rrt.RRT_E_INVALID
    assert host.get_disk() is None


# ------------------------------------------------------------------ round trip
def test_set_get_round_trip(host):
    host.set_disk(7.0, 16.0, emission=EM, temperature=6000.0, profile="zero-torque")
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": EM, "redshift": True,
                               "temperature": 6000.0, "profile": "zero-torque"}
    host.set_disk(7.0, 16.0, emission=EM, temperature=4500.0, redshift=False)
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": EM, "redshift": False,
                               "temperature": 4500.0, "profile": "power"}
    d = rrt.DiskDesc()
    assert rrt.lib().rrt_get_disk(host.h, C.byref(d)) == 1
    assert d.flags == (rrt.RRT_DISK_BLACKBODY | rrt.RRT_DISK_NO_REDSHIFT) and d.temperature == 4500.0 and d.profile == 0
    host.set_disk(None)
    assert host.get_disk() is None


def test_plain_disk_dict_is_unchanged(host):
    host.set_disk(7.0, 16.0, emission=(1.0, 0.5, 0.25), redshift=False)
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": (1.0, 0.5, 0.25), "redshift": False}
    host.set_disk(7.0, 16.0)  # emission=None without a temperature: white
    assert host.get_disk()["emission"] == (1.0, 1.0, 1.0)


def test_default_emission_of_a_blackbody_disk_is_the_tint(host):
    host.set_disk(7.0, 16.0, temperature=6000.0)
    assert host.get_disk()["emission"] == rrt.blackbody_tint(6000.0)


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("temperature", [float("nan"), 999.0, 1e6 + 1.0, -6000.0, float("inf"), 0.0])
def test_invalid_temperatures(host, temperature):
    host.set_disk(7.0, 20.0)
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(temperature=temperature))) == rrt.RRT_E_INVALID
    with pytest.raises(rrt.RRTError) as e:
        host.set_disk(7.0, 16.0, emission=EM, temperature=temperature)
    assert e.value.code == rrt.RRT_E_INVALID
    assert host.get_disk() == {"r_in": 7.0, "r_out": 20.0, "emission": (1.0, 1.0, 1.0), "redshift": True}  # still in force


@pytest.mark.parametrize("temperature", [1000.0, 1e6])
def test_the_range_is_closed(host, temperature):
    host.set_disk(7.0, 16.0, temperature=temperature)
    assert host.get_disk()["temperature"] == temperature


def test_unknown_profile_is_invalid(host):
    host.set_disk(7.0, 20.0)
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(profile=2))) == rrt.RRT_E_INVALID
    assert host.get_disk()["r_out"] == 20.0
    assert rrt.lib().rrt_set_disk(host.h, C.byref(desc(profile=1))) == rrt.RRT_OK


def test_flag_clear_ignores_and_zeroes_the_new_fields(host):
    """Callers that pass garbage where `reserved` was keep working: with the flag clear the two fields are
    not read and are stored as 0."""
    for flags in (0, rrt.RRT_DISK_NO_REDSHIFT):
        d = desc(flags=flags, temperature=float("nan"), profile=0xDEADBEEF)
        d.reserved[0], d.reserved[1] = 0x12345678, 0xFFFFFFFF
        assert rrt.lib().rrt_set_disk(host.h, C.byref(d)) == rrt.RRT_OK
        out = rrt.DiskDesc()
        assert rrt.lib().rrt_get_disk(host.h, C.byref(out)) == 1
        assert bytes(out)[32:48] == bytes(16) and out.flags == flags
        assert set(host.get_disk()) == {"r_in", "r_out", "emission", "redshift"}


def test_disk_eval_errors_need_no_device(host):
    """rrt_disk_eval: without a disk and with a disk invalid for the spacetime RRT_E_INVALID, a valid disk
    gets as far as the device check -- the errors of a render launch, in their order."""
    r, g = np.array([8.0]), np.array([1.0])
    with pytest.raises(rrt.RRTError) as e:
        host.disk_eval(r, g)
    assert e.value.code == rrt.RRT_E_INVALID
    host.set_disk(0.0, 16.0, temperature=6000.0)
    with pytest.raises(rrt.RRTError) as e:  # Schwarzschild kind
        host.disk_eval(r, g)
    assert e.value.code == rrt.RRT_E_INVALID and "spin 0" in str(e.value)
    host.set_black_hole(spin=0.0)
    for n in (1, 0):
        with pytest.raises(rrt.RRTError) as e:
            host.disk_eval(r[:n], g[:n])
        assert e.value.code == rrt.RRT_E_NO_DEVICE
    host.set_disk(5.9, 16.0, temperature=6000.0)
    with pytest.raises(rrt.RRTError) as e:
        host.disk_eval(r, g)
    assert e.value.code == rrt.RRT_E_INVALID and "ISCO" in str(e.value)


# ------------------------------------------------------------------ the tint
def test_tint_green_is_one_and_the_range_is_checked():
    for t in (1000.0, 3000.0, 6500.0, 20000.0, 1e6):
        rgb = rrt.blackbody_tint(t)
        assert rgb[1] == 1.0 and all(math.isfinite(v) and v > 0.0 for v in rgb)
        assert np.allclose(rgb, bb.tint(t), rtol=1e-6)
    for t in (999.9, 1e6 + 1.0, float("nan"), -1.0, float("inf")):
        with pytest.raises(rrt.RRTError) as e:
            rrt.blackbody_tint(t)
        assert e.value.code == rrt.RRT_E_INVALID
    assert rrt.lib().rrt_blackbody_tint(6000.0, None) == rrt.RRT_E_INVALID


def test_tint_reddens_as_it_cools():
    """R / B falls strictly over 1000 .. 1e6 K; 3000 K is orange, 6500 K near white, 20000 K blue."""
    ts = np.geomspace(1000.0, 1e6, 61)
    rb = [rrt.blackbody_tint(t)[0] / rrt.blackbody_tint(t)[2] for t in ts]
    assert all(a > b for a, b in zip(rb, rb[1:])), rb
    r, g, b = rrt.blackbody_tint(3000.0)
    assert r > g > b and r / b > 2.5
    r, g, b = rrt.blackbody_tint(6500.0)
    assert max(r, g, b) / min(r, g, b) < 1.35
    r, g, b = rrt.blackbody_tint(20000.0)
    assert b > g > r


def test_tint_reaches_the_rayleigh_jeans_limit():
    """At 1e6 K the colour is (550 / lambda_c)^4 to 1 %: the first-order correction to the limit is
    |x_G - x_c| / 2 <= 0.0024 with x = K / T."""
    x = [bb.HC_K / lam / 1e6 for lam in bb.LAMBDA]
    assert max(abs(x[1] - v) / 2 for v in x) <= 0.0024
    rgb = rrt.blackbody_tint(1e6)
    for c, lam in enumerate(bb.LAMBDA):
        assert abs(rgb[c] / (550.0 / lam) ** 4 - 1.0) < 0.01


# ------------------------------------------------------------------ the checker's rule, pinned
def test_pin_power_profile_at_r_in_returns_the_emission():
    """POWER at r = r_in, g = 1: c = 1, T_obs = temperature, so x is the quotient the host formed N_c
    from and ratio == 1.0 exactly: emission bit for bit, at any temperature."""
    for t in (1000.0, 3456.75, 6000.0, 1e6):
        hole, disk = hole_and_disk(bb.POWER, temperature=t)
        got = bb.rgb(disk, disk.r_in, 1.0)
        assert got.view(np.uint32).tolist() == np.asarray(EM, np.float32).view(np.uint32).tolist()
        q, temp = bb.temperature(disk, disk.r_in)
        assert q == 1.0 and temp == disk.temperature


def test_pin_zero_torque_profile():
    """Black at r_in; T = temperature to 1e-12 at r = 49/36 r_in, the peak; T falls strictly beyond it (and
    rises strictly up to it)."""
    hole, disk = hole_and_disk(bb.ZERO_TORQUE)
    assert not bb.rgb(disk, disk.r_in, 1.0).any()
    assert bb.temperature(disk, disk.r_in) == (0.0, None)
    r_peak = disk.r_in * 49.0 / 36.0
    assert abs(bb.temperature(disk, r_peak)[1] / disk.temperature - 1.0) < 1e-12
    out = [bb.temperature(disk, r_peak * f)[1] for f in np.geomspace(1.0, 8.0, 40)]
    assert all(a > b for a, b in zip(out, out[1:]))
    inner = [bb.temperature(disk, disk.r_in + (r_peak - disk.r_in) * f)[1] for f in np.linspace(0.02, 1.0, 40)]
    assert all(a < b for a, b in zip(inner, inner[1:]))
    assert np.allclose(bb.rgb(disk, r_peak, 1.0), EM, rtol=1e-6)


def test_pin_power_profile_is_the_plain_disks_flux():
    """T^4 follows the plain disk's (r_in / r)^3."""
    hole, disk = hole_and_disk(bb.POWER)
    for f in (1.0, 1.7, 3.0, 6.5):
        q, t = bb.temperature(disk, disk.r_in * f)
        assert abs((t / disk.temperature) ** 4 * f ** 3 - 1.0) < 1e-12


@pytest.mark.parametrize("profile", [bb.POWER, bb.ZERO_TORQUE])
def test_pin_redshift_moves_the_colour(profile):
    """g < 1 lowers B / R and dims every channel, g > 1 raises both; with RRT_DISK_NO_REDSHIFT g is ignored."""
    hole, disk = hole_and_disk(profile)
    flat = bb.Disk(hole, dc.isco(0.9), 16.0, EM, False, 6000.0, profile)
    for r in (disk.r_in * 1.5, disk.r_in * 4.0):
        lo, mid, hi = (bb.rgb(disk, r, g).astype(np.float64) for g in (0.7, 1.0, 1.4))
        assert lo[2] / lo[0] < mid[2] / mid[0] < hi[2] / hi[0]
        assert (lo < mid).all() and (mid < hi).all()
        assert all(bb.rgb(flat, r, g).tobytes() == mid.astype(np.float32).tobytes() for g in (0.7, 1.0, 1.4, 0.0, math.nan))


@pytest.mark.parametrize("profile", [bb.POWER, bb.ZERO_TORQUE])
def test_pin_degenerate_inputs_are_black(profile):
    hole, disk = hole_and_disk(profile)
    r = disk.r_in * 2.0
    for g in (0.0, -0.0, -1.0, math.inf, -math.inf, math.nan):
        assert not bb.rgb(disk, r, g).any(), g
    for bad in (0.0, -r, math.nan, math.inf):
        assert not bb.rgb(disk, bad, 1.0).any(), bad
    # a tiny T_obs overflows exp: the ratio is N / inf = 0; a huge one leaves a finite colour
    assert not bb.rgb(disk, r, 1e-3).any()
    assert np.isfinite(bb.rgb(disk, r, 3.0)).all() and bb.rgb(disk, r, 3.0).all()


def test_every_intermediate_stays_inside_float_over_the_range():
    """Temperatures 1000 .. 1e6 K, g in (0.05, 3), the whole annulus: every channel is finite."""
    for t in (1000.0, 1e6):
        for profile in (bb.POWER, bb.ZERO_TORQUE):
            hole, disk = hole_and_disk(profile, temperature=t)
            for r in np.geomspace(disk.r_in, 16.0 * hole.m, 9):
                for g in (0.05, 1.0, 3.0):
                    assert np.isfinite(bb.rgb(disk, float(r), g)).all(), (t, profile, r, g)
