"""The thin accretion disk (rrt_set_disk, RRT_RAY_DISK) on the CPU: the host
interface on a host-only context (validation, rrt_get_disk, the resolved ISCO, every error that needs
no device), and the rule of tests/disk_check.py pinned by physics on restated chains before
tests/test_gpu_disk.py compares the GPU with it bit for bit."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import disk_check as dc
import oracle_lib as ol
import rrt
import trace_check as tc
from golden_cases import GOLD, Case

SPHERES = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
M = 0.05
HOLE = (0.0, 1.0, 0.0)


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


# ------------------------------------------------------------------ the host interface
def test_exports_and_layout():
    L = rrt.lib()
    assert "rrt_set_disk" in rrt.EXPORTS and "rrt_get_disk" in rrt.EXPORTS
    assert hasattr(L, "rrt_set_disk") and hasattr(L, "rrt_get_disk")
    assert C.sizeof(rrt.DiskDesc) == 48 and rrt.RRT_RAY_DISK == 4 and rrt.RRT_DISK_NO_REDSHIFT == 1
    assert L.rrt_abi_version() == 5  # additive: the ABI version stays


def test_set_get_remove(host):
    assert host.get_disk() is None
    host.set_disk(7.0, 16.0, emission=(1.0, 0.5, 0.25), redshift=False)
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": (1.0, 0.5, 0.25), "redshift": False}
    host.set_disk(None)
    assert host.get_disk() is None
    assert rrt.lib().rrt_get_disk(host.h, None) == 0


@pytest.mark.parametrize("spin,want,digits", [(0.0, 6.0, 12), (0.5, 4.2330, 4), (0.9, 2.3209, 4)])
def test_resolved_isco(host, spin, want, digits):
    """r_in = 0 is the prograde ISCO of the spin in force when the disk is read (Bardeen's closed form):
    6 M at a = 0, 4.2330 M at 0.5, 2.3209 M at 0.9; a later rrt_set_spacetime re-resolves it."""
    host.set_disk(0.0, 16.0)
    assert host.get_disk()["r_in"] == 0.0  # Schwarzschild kind: nothing to resolve against
    host.set_black_hole(spin=spin)
    got = host.get_disk()["r_in"]
    assert round(got, digits) == want and abs(got - dc.isco(spin)) < 1e-12, got
    host.set_black_hole(spin=0.0)
    assert round(host.get_disk()["r_in"], 12) == 6.0


@pytest.mark.parametrize("r_in,r_out,emission", [
    (float("nan"), 16.0, (1, 1, 1)), (1.0, float("inf"), (1, 1, 1)), (-1.0, 16.0, (1, 1, 1)), (7.0, -16.0, (1, 1, 1)),
    (7.0, 16.0, (1, float("nan"), 1)), (7.0, 16.0, (1, 1, -0.5)), (7.0, 16.0, (float("inf"), 1, 1)),
    (16.0, 16.0, (1, 1, 1)), (16.0, 7.0, (1, 1, 1)), (0.0, 0.0, (1, 1, 1))])
def test_invalid_descriptors(host, r_in, r_out, emission):
    host.set_disk(7.0, 20.0)
    with pytest.raises(rrt.RRTError) as e:
        host.set_disk(r_in, r_out, emission=emission)
    assert e.value.code == rrt.RRT_E_INVALID
    assert host.get_disk()["r_out"] == 20.0  # a rejected descriptor leaves the disk in force


def test_unknown_flags_are_invalid(host):
    d = rrt.DiskDesc()
    d.r_in, d.r_out, d.flags = 7.0, 16.0, 2
    assert rrt.lib().rrt_set_disk(host.h, C.byref(d)) == rrt.RRT_E_INVALID


RAY = (np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, -1.0]]))


def test_launch_time_errors_need_no_device(host):
    """At render or trace time: a Schwarzschild-kind spacetime (the message points to Kerr with spin 0),
    an r_in below the ISCO of the current spin, an r_out at or below the resolved ISCO -- all reported
    before the device is asked for; a valid disk gets as far as the device check."""
    host.set_scene(rrt.SceneFile(SPHERES))
    c = Case("spheres_96x72_s1")
    host.set_camera(rrt.load_camera(c.camera_path))
    p = rrt.render_params(c.frame_w, c.frame_h, ns_aa=1)

    def both(code, text=None):
        for call in (lambda: host.trace_rays(*RAY), lambda: host.trace_camera(96, 72, 0, 0, 96, 72),
                     lambda: host.render(p, 0, 0, 8, 8)):
            with pytest.raises(rrt.RRTError) as e:
                call()
            assert e.value.code == code, str(e.value)
            assert text is None or text in str(e.value), str(e.value)

    host.set_disk(0.0, 16.0)
    host.set_black_hole()
    both(rrt.RRT_E_INVALID, "spin 0")
    host.set_black_hole(spin=0.0)
    both(rrt.RRT_E_NO_DEVICE)
    host.set_disk(5.9, 16.0)       # below 6 M at a = 0 ...
    both(rrt.RRT_E_INVALID, "ISCO")
    host.set_black_hole(spin=0.9)  # ... but outside 2.3209 M at a = 0.9
    both(rrt.RRT_E_NO_DEVICE)
    host.set_disk(2.0, 16.0)
    both(rrt.RRT_E_INVALID, "ISCO")
    host.set_disk(0.0, 5.0)        # r_out inside the ISCO of a = 0
    both(rrt.RRT_E_NO_DEVICE)
    host.set_black_hole(spin=0.0)
    both(rrt.RRT_E_INVALID, "r_out")
    host.set_disk(None)
    both(rrt.RRT_E_NO_DEVICE)
    host.set_black_hole()
    both(rrt.RRT_E_NO_DEVICE)


# ------------------------------------------------------------------ the numpy kerr_init
@pytest.mark.parametrize("kerr", [(0.0, (0.0, 1.0, 0.0)), (0.9, (0.3, 1.0, -0.2)), (0.5, (0.0, 0.0, 1.0))])
def test_kerr_init_gives_a_null_covector(kerr):
    """|H| below 1e-12 of |p|^2 for rays from everywhere in and around the room, and the restated
    chain's first row continues it: L_z of (q0, p0) is the chain's L_z."""
    hole = dc.Hole(tc.DEFAULT_BH, kerr)
    worst = 0.0
    for name, (o, d) in tc.ray_sets(64).items():
        for i in range(len(o)):
            q, p = dc.kerr_init(hole, o[i], d[i])
            H, pp = dc.hamiltonian(hole, q, p)
            worst = max(worst, abs(H) / pp)
            rows, _ = ol.kerr_chain(hole.bh, kerr[0], kerr[1], o[i], d[i], max_rows=1)
            lz0 = q[0] * p[1] - q[1] * p[0]
            lz1 = rows[0, 8] * rows[0, 12] - rows[0, 9] * rows[0, 11]
            # test_kerr_oracle.py's bound on the march's own drift of L_z
            assert abs(lz1 - lz0) < 1e-5 * max(abs(lz0), 1e-3), (name, i, lz0, lz1)
    print(f"a/M = {kerr[0]}: max |H| / |p|^2 = {worst:.2e}")
    assert worst < 1e-12


# ------------------------------------------------------------------ physics pins
def ring_rays(cam, r_m, n, hole):
    """n rays from world point cam to the equatorial ring of radius r_m (in M), evenly in azimuth."""
    ph = 2 * np.pi * (np.arange(n) + 0.5) / n
    ex, ey, c = np.array(hole.ex), np.array(hole.ey), np.array(hole.c)
    tgt = c + (r_m * hole.m) * (np.cos(ph)[:, None] * ex + np.sin(ph)[:, None] * ey)
    o = np.repeat(np.asarray(cam, np.float64)[None], n, 0)
    return o, tc.unit(tgt - o)


def first_crossings(bh, kerr, o, d, r_out=40.0):
    """(hole, disk, per ray its first crossing on the annulus ISCO..r_out, or None)."""
    hole = dc.Hole(bh, kerr)
    disk = dc.Disk(hole, dc.isco(kerr[0]), r_out)
    return hole, disk, [dc.first_on(dc.crossings(hole, disk, o[i], d[i])) for i in range(len(o))]


def bh_dt(dt):
    return HOLE + (2 * M, dt)


def test_pin_axis_camera_schwarzschild():
    """a = 0, camera on the axis: every photon has L_z = 0, so g = 1 / u^t = sqrt(1 - 3M / r) at the
    radius it crosses at."""
    kerr = (0.0, (0.0, 1.0, 0.0))
    for r_m in (9.0, 12.0, 25.0):
        hole, disk, cs = first_crossings(bh_dt(0.1), kerr, *ring_rays((0.0, 1.9, 0.0), r_m, 16, dc.Hole(bh_dt(0.1), kerr)))
        for c in cs:
            assert c is not None
            print(f"aimed {r_m} M: r = {c.r / hole.m:.3f} M, L_z = {c.lz:.1e}, g = {c.g:.6f}")
            assert abs(c.lz) < 1e-12 * M and c.side == 1.0
            assert abs(c.g - math.sqrt(1.0 - 3.0 * hole.m / c.r)) < 1e-12
            assert 0.7 * r_m < c.r / hole.m < r_m  # the ray bends inward of the aimed ring


def exact_g(hole, disk, q, p, r):
    """g from the conserved L_z of the ray's initial state at radius r."""
    return dc.redshift(hole, disk, r, q[0] * p[1] - q[1] * p[0])


def inclined(kerr, dt):
    """Rays from a camera 60 degrees off the axis, 24 M out, to the ring r = 10 M; those that land on the
    near half of the ring (the far side's rays pass the hole first): (hole, disk, crossings, the
    crossings' deviation |g - g_exact|), g_exact from the initial state's conserved L_z at the radius
    the fine march (dtheta = 0.005) crosses at."""
    h0 = dc.Hole(bh_dt(dt), kerr)
    cam = np.array(h0.c) + 1.2 * (math.sin(math.radians(60)) * np.array(h0.ex) + math.cos(math.radians(60)) * np.array(h0.ez))
    o, d = ring_rays(cam, 10.0, 24, h0)
    hole, disk, cs = first_crossings(bh_dt(dt), kerr, o, d)
    _, _, fine = first_crossings(bh_dt(0.005), kerr, o, d)
    keep, dev = [], []
    for i, c in enumerate(cs):
        if c is None or fine[i] is None or abs(fine[i].r / hole.m - 10.0) > 2.5:
            continue
        q, p = dc.kerr_init(hole, o[i], d[i])
        keep.append(c)
        dev.append(abs(c.g - exact_g(hole, disk, q, p, fine[i].r)))
    assert len(keep) >= 12
    return hole, disk, keep, np.array(dev)


# |g - g_exact| of the inclined pins at dtheta = 0.1, measured (0.1 -> 0.04 falls by
# the square of the step ratio), with the factor 2 the interpolation rule's tolerance takes
PIN_DEV_01 = {0.0: 1.179e-4, 0.9: 1.101e-4}


@pytest.mark.parametrize("spin", [0.0, 0.9])
def test_pin_interpolation_error_is_second_order(spin):
    """Linear interpolation between the step's end states leaves an error of order dtheta^2: the pins'
    deviation falls by about (0.1 / 0.04)^2 = 6.25 from dtheta = 0.1 to 0.04 (first order would give
    2.5, third 15.6), and at 0.1 it stays within twice the measured value."""
    kerr = (spin, (0.0, 1.0, 0.0))
    d01 = inclined(kerr, 0.1)[3].max()
    d004 = inclined(kerr, 0.04)[3].max()
    print(f"a/M = {spin}: max |g - g_exact| = {d01:.3e} at dtheta 0.1, {d004:.3e} at 0.04, ratio {d01 / d004:.2f}")
    assert 4.0 < d01 / d004 < 10.0
    assert d01 <= 2.0 * PIN_DEV_01[spin]


def test_pin_inclined_view_schwarzschild():
    """a = 0, camera 60 degrees off the axis: at (nearly) equal r the side with L_z > 0 is the brighter."""
    hole, disk, cs, dev = inclined((0.0, (0.0, 1.0, 0.0)), 0.1)
    pos = [c for c in cs if c.lz > 0.5 * M]
    neg = [c for c in cs if c.lz < -0.5 * M]
    assert len(pos) >= 6 and len(neg) >= 6
    rs = np.array([c.r for c in cs]) / hole.m
    assert rs.max() - rs.min() < 2.5, rs  # the ring stays a ring
    assert min(c.g for c in pos) > max(c.g for c in neg)
    # against the rest-frame value of that radius: blue on one side, red on the other
    for c in pos + neg:
        rest = math.sqrt(1.0 - 3.0 * hole.m / c.r)
        assert (c.g > rest) == (c.lz > 0)


def test_pin_prograde_side_is_the_bright_side():
    """a/M = 0.9: the sign of L_z that is prograde is the one test_kerr_oracle.py's critical impact
    parameters give -- a ray along +ex at y < 0 has L_z = -y p_x > 0 and is captured only inside
    2.84 M (the prograde side; 6.83 M on the other) -- and that side of the disk is the bright one."""
    spin = 0.9
    kerr = (spin, (0.0, 1.0, 0.0))
    a = spin * M
    b_pro = -a + 6 * M * np.cos(np.arccos(-spin) / 3)
    b_ret = a + 6 * M * np.cos(np.arccos(spin) / 3)
    assert round(b_pro / M, 2) == 2.84 and round(b_ret / M, 2) == 6.83
    hole = dc.Hole(bh_dt(0.02), kerr)
    ex, ey = np.array(hole.ex), np.array(hole.ey)
    for b, want_captured in [(1.05 * b_pro, 0), (0.95 * b_pro, 1)]:
        o = np.array(HOLE) - 2.0 * ex - b * ey  # y = -b < 0
        q, p = dc.kerr_init(hole, o, ex)
        assert q[0] * p[1] - q[1] * p[0] > 0  # L_z > 0 ...
        rows, _ = ol.kerr_chain(hole.bh, spin, kerr[1], o, ex, max_rows=4000)
        assert rows[-1, 7] == want_captured  # ... and the capture threshold is the prograde one
    o = np.array(HOLE) - 2.0 * ex + 3.5 * M * ey  # y > 0: L_z < 0, inside 6.83 M: captured
    rows, _ = ol.kerr_chain(hole.bh, spin, kerr[1], o, ex, max_rows=4000)
    assert rows[-1, 7] == 1
    hole, disk, cs, dev = inclined(kerr, 0.1)
    pos = [c for c in cs if c.lz > 0.5 * M]
    neg = [c for c in cs if c.lz < -0.5 * M]
    assert len(pos) >= 6 and len(neg) >= 6
    assert min(c.g for c in pos) > max(c.g for c in neg)
    assert max(c.g for c in pos) > 1.0 > max(c.g for c in neg)  # beamed blue against red


def test_radiance_formula():
    """rgb = emission x (float)((r_in / r)^3 x g^4); without redshift g = 1 and |n| = 1."""
    kerr = (0.9, (0.3, 1.0, -0.2))
    hole = dc.Hole(tc.DEFAULT_BH, kerr)
    o, d = dc.annulus_rays(hole, 3.0, 15.0, n=32)
    em = (2.0, 1.0, 0.5)
    for redshift in (True, False):
        disk = dc.Disk(hole, dc.isco(0.9), 16.0, em, redshift)
        seen = 0
        for i in range(len(o)):
            c = dc.first_on(dc.crossings(hole, disk, o[i], d[i]))
            if c is None:
                continue
            seen += 1
            g = c.g if redshift else 1.0
            assert np.allclose(c.rgb, np.array(em) * (disk.r_in / c.r) ** 3 * g ** 4, rtol=1e-6)
            assert abs(np.linalg.norm(c.n) - g) < 1e-12 and (c.n @ np.array(hole.ez)) * c.side > 0
            assert redshift or c.g == 1.0
        assert seen >= 16


# ------------------------------------------------------------------ the GPU tests' ray sets
@pytest.mark.parametrize("rset", dc.GPU_SETS)
def test_gpu_ray_sets_exercise_the_rule(rset):
    """Every ray set tests/test_gpu_disk.py traces must show, by the CPU rule alone, at least 32 DISK
    records, 8 rays that cross the plane off the annulus and go on, and 4 rows that hold both an annulus
    crossing and the ray's primitive hit.  The first two hold under each hole with the ISCO..16 M disk.
    With that disk no chord can hold a crossing and a hit -- the annulus stays 0.23 from the nearest
    primitive and no chord there is longer than 0.09 -- so the GPU test traces every set with the
    ISCO..30 M disk too, which reaches the walls and still lies inside the room's bounding sphere, and
    the contests are counted there, over the holes the set is traced under (the tilted disk hides its
    own junction with the walls from the camera; the upright one shows 7)."""
    prims = tc.Prims(rrt.SceneFile(SPHERES))
    contests = 0
    for kerr in sorted(dc.KERRS):
        hole = dc.Hole(tc.DEFAULT_BH, dc.KERRS[kerr])
        o, d = dc.gpu_rays(rset, hole)
        orc = tc.Oracle(SPHERES, tc.DEFAULT_BH, dc.KERRS[kerr])
        answers = orc.query(o, d)
        r_in = dc.isco(dc.KERRS[kerr][0])
        n16 = dc.cpu_counts(orc, prims, hole, dc.Disk(hole, r_in, dc.R_OUT), o, d, answers)
        n30 = dc.cpu_counts(orc, prims, hole, dc.Disk(hole, r_in, dc.R_OUT_WIDE), o, d, answers)
        print(f"{rset}/{kerr}: 16 M {n16}, 30 M {n30}")
        assert n16["disk"] >= 32 and n16["through"] >= 8 and n16["contest"] == 0, n16
        assert n30["disk"] >= 32, n30
        contests += n30["contest"]
        # both disks lie inside the room's bounding sphere about the hole: r_esc2 keeps its value
        assert (dc.R_OUT_WIDE * hole.m) ** 2 + hole.a2 < 1.0 + 1.0 + 1.0  # the farthest corner's |.|^2
    assert contests >= 4, contests
