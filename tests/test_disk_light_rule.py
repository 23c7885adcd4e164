"""The disk light (RRT_DISK_LIGHT, rrt_disk_sample) on the CPU: the host interface on a
host-only context, the rule of tests/disk_light_check.py pinned by geometry before
tests/test_gpu_disk_light.py compares the GPU with it bit for bit, and, by the CPU rule alone, the counts
that make that test's pixel set adequate."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import disk_check as dc
import disk_light_check as lc
import rrt
import trace_check as tc
from golden_cases import GOLD, Case

SPHERES = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
BH = tc.DEFAULT_BH


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


def light_of(kerr, r_out=dc.R_OUT):
    hole = dc.Hole(BH, dc.KERRS[kerr])
    return lc.Light(hole, dc.Disk(hole, dc.isco(dc.KERRS[kerr][0]), r_out))


# ------------------------------------------------------------------ the host interface
def test_exports_flag_and_layout(host):
    L = rrt.lib()
    assert "rrt_disk_sample" in rrt.EXPORTS and hasattr(L, "rrt_disk_sample")
    assert rrt.RRT_DISK_LIGHT == 16 and C.sizeof(rrt.DiskDesc) == 48 and L.rrt_abi_version() == 5
    host.set_disk(7.0, 16.0, light=True)
    assert host.get_disk() == {"r_in": 7.0, "r_out": 16.0, "emission": (1.0, 1.0, 1.0), "redshift": True, "light": True}
    d = rrt.DiskDesc()
    assert L.rrt_get_disk(host.h, C.byref(d)) == 1 and d.flags == rrt.RRT_DISK_LIGHT
    host.set_disk(7.0, 16.0, temperature=6000.0, redshift=False, light=True)
    assert L.rrt_get_disk(host.h, C.byref(d)) == 1
    assert d.flags == rrt.RRT_DISK_LIGHT | rrt.RRT_DISK_BLACKBODY | rrt.RRT_DISK_NO_REDSHIFT
    host.set_disk(7.0, 16.0)
    assert "light" not in host.get_disk()  # without the flag the dict is what it was
    for flags in (2, 8, 2 | rrt.RRT_DISK_LIGHT, 8 | rrt.RRT_DISK_LIGHT, 32):  # bits 1 and 3 stay unassigned, with the new bit too
        d = rrt.DiskDesc()
        d.r_in, d.r_out, d.flags = 7.0, 16.0, flags
        assert L.rrt_set_disk(host.h, C.byref(d)) == rrt.RRT_E_INVALID


def test_disk_sample_errors_need_no_device(host):
    """rrt_disk_eval's: no disk and a Schwarzschild-kind spacetime are RRT_E_INVALID, a disk invalid for
    the spin too; a valid disk, with or without the flag, gets as far as the device check."""
    p, uv = np.array([[0.2, 0.3, 0.1]]), np.array([[0.5, 0.5]])
    host.set_black_hole(spin=0.5)

    def code():
        with pytest.raises(rrt.RRTError) as e:
            host.disk_sample(p, uv)
        return e.value.code, str(e.value)

    assert code()[0] == rrt.RRT_E_INVALID
    for light in (False, True):
        host.set_disk(0.0, 16.0, light=light)
        assert code()[0] == rrt.RRT_E_NO_DEVICE
    host.set_black_hole()
    c, text = code()
    assert c == rrt.RRT_E_INVALID and "spin 0" in text
    host.set_black_hole(spin=0.0)
    host.set_disk(5.0, 16.0)
    c, text = code()
    assert c == rrt.RRT_E_INVALID and "ISCO" in text
    with pytest.raises(ValueError):
        host.disk_sample(np.zeros((2, 3)), np.zeros((1, 2)))


# ------------------------------------------------------------------ the rule, pinned
DRAWS = (0.0, 1.0, 0.5, 1.0 / 2147483647.0, 2147483646.0 / 2147483647.0, 0.25, 0.123456789)


@pytest.mark.parametrize("r_out", [dc.R_OUT, dc.R_OUT_WIDE])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_sampled_points_lie_on_the_annulus(kerr, r_out):
    """r_in^2 <= x^2 + y^2 - a^2 <= r_out^2 for every pair of the draws, 0 and 1 among them, to 1e-12
    relative (a dozen roundings of 2^-53 from the stored squares to the sum of the two squares), and the
    world point wi aims at is the point: p + d wi returns to it, in the plane through the hole's centre."""
    light = light_of(kerr, r_out)
    hole, disk = light.hole, light.disk
    p = [0.3, 0.2, -0.4]
    for u in DRAWS:
        for v in DRAWS:
            x, y = lc.point(light, u, v)
            r2 = (x * x + y * y) - hole.a2
            assert disk.r_in2 * (1 - 1e-12) <= r2 <= disk.r_out2 * (1 + 1e-12), (u, v, r2)
            ok, wi, pdf = lc.sample(light, p, u, v)
            P = np.array(lc.world(hole, x, y, 0.0))
            assert ok and abs(np.linalg.norm(wi) - 1.0) < 1e-15
            dist = np.linalg.norm(P - p)
            assert np.abs(np.array(p) + dist * np.array(wi) - P).max() < 1e-14
            assert abs((P - hole.c) @ np.array(hole.ez)) < 1e-15
    # u picks the radius monotonically: 0 the inner edge, 1 the outer
    x0, y0 = lc.point(light, 0.0, 0.0)
    x1, y1 = lc.point(light, 1.0, 0.0)
    assert abs(x0 * x0 + y0 * y0 - light.rho_in2) <= 1e-15 * light.rho_in2
    assert abs(x1 * x1 + y1 * y1 - (disk.r_out2 + hole.a2)) <= 1e-15 * (disk.r_out2 + hole.a2)


@pytest.mark.parametrize("height", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_pdf_integrates_to_the_flat_solid_angle(kerr, height):
    """The density is d^2 / (area |cos|) over the flat image, so the mean of 1 / pdf over uniform draws is
    the image's solid angle.  From a point on the axis at height h that is, in closed form,
    2 pi h (1 / sqrt(h^2 + rho_in^2) - 1 / sqrt(h^2 + rho_out^2)), rho the Kerr-Schild radii.  There the
    integrand does not depend on v and is f(u) = area h s^-3/2, s = h^2 + rho_in^2 + u span, so
    f'''' / f = (945 / 16) (span / s)^4 <= 59 x 36^4 = 1e8 for these disks and heights; Simpson's rule
    over 4096 intervals of u errs by at most that / (180 x 4096^4) = 2e-9 relative, and each float pdf by
    2^-24 = 6e-8: 1e-6 relative is asked."""
    light = light_of(kerr)
    hole = light.hole
    assert light.rho_span / (height * height + light.rho_in2) < 36.0
    p = [hole.c[i] + height * hole.ez[i] for i in range(3)]
    n = 4096
    inv = []
    for k in range(n + 1):
        ok, wi, pdf = lc.sample(light, p, k / n, 0.37)
        assert ok
        inv.append((1.0 if k in (0, n) else 4.0 if k % 2 else 2.0) / float(pdf))
    for v in (0.0, 0.11, 0.5, 0.93):  # no dependence on the azimuth
        assert abs(float(lc.sample(light, p, 0.5, v)[2]) / float(lc.sample(light, p, 0.5, 0.37)[2]) - 1.0) < 1e-6
    rho_out2 = light.rho_in2 + light.rho_span
    omega = 2.0 * math.pi * height * (1.0 / math.sqrt(height * height + light.rho_in2) - 1.0 / math.sqrt(height * height + rho_out2))
    got = sum(inv) / (3.0 * n)
    print(f"{kerr} h={height}: mean 1/pdf {got:.9f}, solid angle {omega:.9f}")
    assert abs(got / omega - 1.0) < 1e-6


def test_a_point_in_the_plane_is_invalid():
    """With the axis along +y the plane is y = c_y exactly: every sampled point has that y, dv.y is 0, the
    cosine 0 and the density infinite -- disk_sample returns false, for every draw."""
    light = light_of("a0")
    cy = light.hole.c[1]
    for p in ([0.3, cy, -0.2], [2.0, cy, 0.0], [-0.01, cy, 0.7]):
        for u in DRAWS:
            for v in DRAWS:
                ok, wi, pdf = lc.sample(light, p, u, v)
                assert not ok and np.isinf(pdf)
    wi, pdf = lc.sample_many(light, [[0.3, cy, -0.2]], [[0.5, 0.5]])
    assert pdf[0] == 0.0  # rrt_disk_sample's report of an invalid sample
    ok, _, pdf = lc.sample(light, [0.3, cy + 1e-9, -0.2], 0.5, 0.5)
    assert ok and np.isfinite(pdf)  # just off the plane: valid, and large
    # the sampled point itself: 0 / 0
    x, y = lc.point(light, 0.5, 0.5)
    ok, wi, pdf = lc.sample(light, lc.world(light.hole, x, y, 0.0), 0.5, 0.5)
    assert not ok


@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_pdf_is_symmetric_under_the_mirror_image(kerr):
    """Both faces emit: p and its mirror image in the disk's plane get the same density.  With the axis
    along +y and p.y - c_y exact the two computations differ by one sign: the bits agree; with the tilted
    axis the image is rounded: 1e-6 relative (the float's 2^-24 and a few 2^-53)."""
    light = light_of(kerr)
    hole = light.hole
    ez, c = np.array(hole.ez), np.array(hole.c)
    g = np.random.default_rng(3)
    for _ in range(64):
        p = c + np.array([g.uniform(-0.9, 0.9), 0.25 * g.integers(1, 3), g.uniform(-0.9, 0.9)])
        q = p - 2.0 * ((p - c) @ ez) * ez
        u, v = g.random(2)
        ok_p, wp, fp = lc.sample(light, p, u, v)
        ok_q, wq, fq = lc.sample(light, q, u, v)
        assert ok_p and ok_q
        if kerr == "a0":
            assert fp.tobytes() == fq.tobytes() and wp[0] == wq[0] and wp[1] == -wq[1] and wp[2] == wq[2]
        else:
            assert abs(float(fp) / float(fq) - 1.0) < 1e-6


# ------------------------------------------------------------------ the GPU pixel test's inputs
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_the_pixel_set_is_adequate(kerr):
    """By the CPU rule alone: of the pixels tests/test_gpu_disk_light.py looks at (every STRIDE-th of the
    96 x 72 frame through the wide camera), at least 300 are checked -- their camera ray ends on a
    diffuse surface with an axis-aligned normal -- and their 4 light samples each make at least 200
    shadow rays that end on the DISK and at least 50 that a primitive or a capture stops."""
    hole = dc.Hole(BH, dc.KERRS[kerr])
    disk = dc.Disk(hole, dc.isco(dc.KERRS[kerr][0]), dc.R_OUT)
    light = lc.Light(hole, disk)
    scene = rrt.SceneFile(SPHERES)
    bsdfs = lc.bsdfs_of(scene)
    first_draw = lc.n_listed_draws(scene, lc.NS_AREA_LIGHT)
    assert first_draw == 2 * lc.NS_AREA_LIGHT  # CBspheres: one area light
    orc = tc.Oracle(SPHERES, BH, dc.KERRS[kerr])
    xs, ys = lc.frame_pixels()
    o, d = lc.camera_rays(Case(lc.WIDE_CASE).camera_path, xs, ys)
    ans = orc.query(o, d)
    n = {"pixels": 0, "samples": 0, "invalid": 0, "behind": 0, "disk": 0, "prim": 0, "capture": 0, "none": 0}
    for i in range(len(o)):
        hit, hp, nn, bsdf = ans[i]
        if not hit or not lc.checkable(bsdfs, bsdf, nn) or lc.cpu_outcome(hole, disk, o[i], d[i], ans[i]) != "prim":
            continue
        n["pixels"] += 1
        key = lc.ol.lib().ro_pixel_key(0, int(xs[i]), int(ys[i]))
        for s in lc.pixel_samples(light, hp, nn, key, first_draw, lc.NS_AREA_LIGHT):
            n["samples"] += 1
            if not s.ok:
                n["invalid"] += 1
            elif not s.shadow:
                n["behind"] += 1
            else:
                so, sd = np.array(s.o), np.array(s.wi)
                n[lc.cpu_outcome(hole, disk, so, sd, orc.query(so[None], sd[None])[0])] += 1
    print(f"{kerr}: {n}")
    assert n["pixels"] >= 300 and n["disk"] >= 200 and n["prim"] + n["capture"] >= 50, n
