"""The moving observer (rrt_set_observer) on the CPU: the host interface on a host-only
context (validation, rrt_get_observer and its resolved constants against tests/observer_check.py bit for
bit, every error that needs no device), and the rule of tests/observer_check.py pinned by physics --
the static tetrad, the photon kerr_init builds from d_eff, its energy in the camera's frame, the flat
limit's aberration and Doppler formulae -- before tests/test_gpu_observer.py compares the GPU with it
bit for bit."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import disk_check as dc
import observer_check as oc
import rrt
import trace_check as tc
from golden_cases import GOLD, Case

SPHERES = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
BH = tc.DEFAULT_BH
CAMERAS = ("case", "6M")  # the case's camera; the same camera moved to 6 M from the hole
W, H = 96, 72


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


def camera(which, hole):
    cam = rrt.load_camera(Case(dc.CAMERA_CASE).camera_path)
    if which == "6M":
        p = oc.moved_position(hole, list(cam.pos), 6.0)
        cam.pos[0], cam.pos[1], cam.pos[2] = p
    return cam


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ the host interface
def test_exports_and_layout():
    L = rrt.lib()
    for name in ("rrt_set_observer", "rrt_get_observer", "rrt_observer_eval"):
        assert name in rrt.EXPORTS and hasattr(L, name)
    assert C.sizeof(rrt.ObserverDesc) == 48
    assert (rrt.RRT_OBSERVER_FRAME_STATIC, rrt.RRT_OBSERVER_FRAME_COORDINATE, rrt.RRT_OBSERVER_NO_BEAMING) == (0, 1, 1)
    assert L.rrt_abi_version() == 5  # additive: the ABI version stays


def test_set_get_remove(host):
    assert host.get_observer() is None
    host.set_observer((0.25, -0.5, 0.125), frame="coordinate", beaming=False)
    assert host.get_observer() == {"velocity": (0.25, -0.5, 0.125), "frame": "coordinate", "beaming": False}
    host.set_observer((0.0, 0.0, 0.0))
    assert host.get_observer() == {"velocity": (0.0, 0.0, 0.0), "frame": "static", "beaming": True}
    host.set_observer(None)
    assert host.get_observer() is None
    assert rrt.lib().rrt_get_observer(host.h, None, None) == 0


@pytest.mark.parametrize("velocity", [(float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, -float("inf")), (0.9991, 0, 0),
                                      (0.6, 0.6, 0.6), (0, -1.0, 0), (2.0, 0, 0)])
def test_invalid_velocities(host, velocity):
    host.set_observer((0.1, 0.2, 0.3))
    with pytest.raises(rrt.RRTError) as e:
        host.set_observer(velocity)
    assert e.value.code == rrt.RRT_E_INVALID and "observer" in str(e.value)
    assert host.get_observer()["velocity"] == (0.1, 0.2, 0.3)  # a rejected descriptor leaves the one in force


def test_the_speed_limit_is_inclusive(host):
    host.set_observer((0.999, 0.0, 0.0))
    assert host.get_observer()["velocity"][0] == 0.999


@pytest.mark.parametrize("field,value", [("frame", 2), ("frame", 0xffffffff), ("flags", 2), ("flags", 0x80000000),
                                         ("reserved0", 1), ("reserved3", 7)])
def test_invalid_descriptors(host, field, value):
    host.set_observer((0.1, 0.2, 0.3), frame="coordinate")
    d = rrt.ObserverDesc()
    d.velocity[0] = 0.5
    if field.startswith("reserved"):
        d.reserved[int(field[-1])] = value
    else:
        setattr(d, field, value)
    assert rrt.lib().rrt_set_observer(host.h, C.byref(d)) == rrt.RRT_E_INVALID
    assert host.get_observer() == {"velocity": (0.1, 0.2, 0.3), "frame": "coordinate", "beaming": True}


@pytest.mark.parametrize("frame", [oc.STATIC, oc.COORDINATE])
@pytest.mark.parametrize("which", CAMERAS)
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_resolved_constants_are_the_checkers(host, kerr, which, frame):
    """rrt_get_observer's resolved[12] equal tests/observer_check.py's bit for bit; they need a camera and
    a Kerr spacetime, and a later rrt_set_camera / rrt_set_spacetime re-resolves them."""
    k = dc.KERRS[kerr]
    hole = dc.Hole(BH, k)
    cam = camera(which, hole)
    beta = oc.gpu_velocity(list(cam.c2w))
    host.set_observer(beta, frame=frame)
    assert "resolved" not in host.get_observer()  # no camera, no Kerr spacetime yet
    host.set_camera(cam)
    assert "resolved" not in host.get_observer()  # a Schwarzschild-kind spacetime
    host.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1])
    ob = oc.Observer(hole, list(cam.pos), beta, frame)
    res = np.full(12, np.nan)
    assert rrt.lib().rrt_get_observer(host.h, None, res.ctypes.data) == 1
    assert np.array_equal(bits(res), bits(ob.resolved())), (res, ob.resolved())
    got = host.get_observer()["resolved"]
    assert got["f"] == ob.f and got["D_g"] == ob.dg and not got["identity"]
    assert (got["alpha"] == 0.0 and got["D_g"] == 1.0) == (frame == oc.COORDINATE)
    # the camera of the other kind, then another spin: resolved anew
    other = camera(CAMERAS[1 - CAMERAS.index(which)], hole)
    host.set_camera(other)
    assert host.get_observer()["resolved"]["f"] == oc.Observer(hole, list(other.pos), beta, frame).f != ob.f
    host.set_camera(cam)
    host.set_black_hole(BH[:3], BH[3], BH[4], spin=0.5, axis=k[1])
    assert host.get_observer()["resolved"]["f"] == oc.Observer(dc.Hole(BH, (0.5, k[1])), list(cam.pos), beta, frame).f


def test_the_identity_is_flagged(host):
    """FRAME_COORDINATE with beta exactly 0 is the identity; nothing else is."""
    hole = dc.Hole(BH, dc.KERRS["a0.9"])
    cam = camera("case", hole)
    host.set_camera(cam)
    host.set_black_hole(BH[:3], BH[3], BH[4], spin=0.9, axis=dc.KERRS["a0.9"][1])
    for beta, frame, want in (((0, 0, 0), "coordinate", True), ((0, 0, 0), "static", False), ((0, 1e-300, 0), "coordinate", False),
                              ((-0.0, 0.0, -0.0), "coordinate", True)):
        host.set_observer(beta, frame=frame)
        assert host.get_observer()["resolved"]["identity"] == want
        ob = oc.Observer(hole, list(cam.pos), beta, frame)
        assert ob.identity == want
        if want:
            n = tc.unit(np.random.default_rng(2).normal(size=(16, 3)))
            d, dv, dd = oc.observer_ray(ob, n)
            assert np.array_equal(bits(d), bits(n)) and (dv == 1.0).all() and (dd == 1.0).all()


RAY = (np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, -1.0]]))


def test_launch_time_errors_need_no_device(host):
    """With an observer set: a Schwarzschild-kind spacetime and a camera at or inside the static limit are
    refused by render, trace_camera and observer_eval before the device is asked for, with a message naming
    the observer; trace_rays ignores the observer; wave mode is refused; a valid observer gets as far as
    the device check."""
    host.set_scene(rrt.SceneFile(SPHERES))
    hole = dc.Hole(BH, dc.KERRS["a0"])
    cam = camera("case", hole)
    host.set_camera(cam)
    p = rrt.render_params(W, H, ns_aa=1)
    calls = (lambda: host.render(p, 0, 0, 8, 8), lambda: host.trace_camera(W, H, 0, 0, 8, 8),
             lambda: host.observer_eval(RAY[1]))

    def all_calls(code, text=None):
        for call in calls:
            with pytest.raises(rrt.RRTError) as e:
                call()
            assert e.value.code == code, str(e.value)
            assert text is None or text in str(e.value), str(e.value)

    host.set_observer((0.1, 0.0, 0.0))
    host.set_black_hole(BH[:3], BH[3], BH[4])
    all_calls(rrt.RRT_E_INVALID, "observer")
    with pytest.raises(rrt.RRTError) as e:
        host.trace_rays(*RAY)
    assert e.value.code == rrt.RRT_E_NO_DEVICE  # caller rays: the observer is ignored
    host.set_black_hole(BH[:3], BH[3], BH[4], spin=0.0)
    all_calls(rrt.RRT_E_NO_DEVICE)
    with pytest.raises(rrt.RRTError) as e:
        host.trace_camera(W, H, 0, 0, 8, 8, mode="wave")
    assert e.value.code == rrt.RRT_E_INVALID
    # inside the static limit of a = 0 (r = 2 M): 1.9 M from the hole, f = 2 M / r > 1
    inside = oc.moved_position(hole, list(cam.pos), 1.9)
    cam.pos[0], cam.pos[1], cam.pos[2] = inside
    host.set_camera(cam)
    assert host.get_observer()["resolved"]["f"] > 1.0
    all_calls(rrt.RRT_E_INVALID, "observer")
    host.set_observer((0.1, 0.0, 0.0), frame="coordinate")  # no static frame needed
    all_calls(rrt.RRT_E_NO_DEVICE)
    host.set_observer(None)
    with pytest.raises(rrt.RRTError) as e:
        host.observer_eval(RAY[1])
    assert e.value.code == rrt.RRT_E_INVALID and "observer" in str(e.value)


def test_observer_eval_of_nothing_needs_no_device(host):
    host.set_camera(camera("case", dc.Hole(BH, dc.KERRS["a0"])))
    host.set_black_hole(BH[:3], BH[3], BH[4], spin=0.0)
    host.set_observer((0.1, 0.0, 0.0))
    with pytest.raises(rrt.RRTError) as e:
        host.observer_eval(np.zeros((0, 3)))
    assert e.value.code == rrt.RRT_E_NO_DEVICE  # the device check comes before the count, as in rrt_disk_eval


# ------------------------------------------------------------------ physics pins on the checker
RADII = (3.0, 4.5, 6.0, 10.0, 30.0, 100.0)
BETA = (0.4, 0.1, -0.2)


def pin_cases():
    for spin, axis in ((0.0, (0.0, 1.0, 0.0)), (0.9, (0.3, 1.0, -0.2))):
        hole = dc.Hole(BH, (spin, axis))
        for r_m in RADII:
            pos = oc.moved_position(hole, (0.3, 1.4, 2.0), r_m)
            yield spin, r_m, hole, pos


def directions(seed=7, n=256):
    return tc.unit(np.random.default_rng(seed).normal(size=(n, 3)))


def test_the_tetrad_is_orthonormal_and_the_ray_is_null():
    """g(u_s, u_s) = -1, g(e_i, e_j) = delta_ij, g(e_i, u_s) = 0 and u_s + e(n) is null, to 1e-13."""
    worst = 0.0
    for spin, r_m, hole, pos in pin_cases():
        ob = oc.Observer(hole, pos, BETA)
        g = oc.metric(ob)
        u, e = oc.tetrad(ob)
        err = max(abs(u @ g @ u + 1.0), np.abs(e @ g @ e.T - np.eye(3)).max(), np.abs(e @ g @ u).max())
        n, _ = oc.static_direction(ob, directions())
        k = u[None] + n @ e
        err = max(err, np.abs(np.einsum("ni,ij,nj->n", k, g, k)).max())
        worst = max(worst, err)
        assert err < 1e-13, (spin, r_m, err)
    print(f"tetrad / null worst {worst:.2e}")


def test_kerr_init_builds_the_tetrads_photon():
    """dc.kerr_init(d_eff) equals g . (u_s + e(n)) scaled to p_t = -1, to 1e-12, and lies on the photon
    shell of the Hamiltonian to 1e-12: the march needs no change."""
    worst = 0.0
    for spin, r_m, hole, pos in pin_cases():
        ob = oc.Observer(hole, pos, BETA)
        g = oc.metric(ob)
        u, e = oc.tetrad(ob)
        npr = directions()
        n, _ = oc.static_direction(ob, npr)
        d_eff, _, _ = oc.observer_ray(ob, npr)
        for i in range(len(npr)):
            p = g @ (u + n[i] @ e)
            p = p / -p[0]
            q, pl = dc.kerr_init(hole, pos, d_eff[i])
            err = np.abs(np.array(hole.local(p[1:])) - np.array(pl)).max()
            ham = abs(dc.hamiltonian(hole, q, pl)[0])
            worst = max(worst, err, ham)
            assert err < 1e-12 and ham < 1e-12, (spin, r_m, i, err, ham)
    print(f"kerr_init worst {worst:.2e}")


def test_d_is_the_received_photons_energy_in_the_camera_frame():
    """-p . u_cam = D, to 1e-12 relative, with u_cam = gamma (u_s + beta^i e_i) and p the covector (p_t = -1)
    of the photon the camera receives from the viewing direction n: the future-directed null vector
    u_s - e(n), the local time reverse of the marched one (the march runs it backwards).
    Also D_v = D / D_g, and for Schwarzschild D_g = 1 / sqrt(1 - 2M / r)."""
    worst = 0.0
    for spin, r_m, hole, pos in pin_cases():
        ob = oc.Observer(hole, pos, BETA)
        g = oc.metric(ob)
        u, e = oc.tetrad(ob)
        ucam = oc.camera_velocity(ob)
        assert abs(ucam @ g @ ucam + 1.0) < 1e-13
        npr = directions()
        n, _ = oc.static_direction(ob, npr)
        _, dv, dd = oc.observer_ray(ob, npr)
        p = (u[None] - n @ e) @ g
        p = p / -p[:, :1]
        err = np.abs(-(p @ ucam) / dd - 1.0).max()
        worst = max(worst, err)
        assert err < 1e-12, (spin, r_m, err)
        assert np.abs(dd / (ob.dg * dv) - 1.0).max() < 1e-15
        if spin == 0.0:
            assert abs(ob.dg * math.sqrt(1.0 - 2.0 / r_m) - 1.0) < 1e-12, (r_m, ob.dg)
            assert abs(ob.r / hole.m - r_m) < 1e-9
    print(f"-p.u_cam / D - 1 worst {worst:.2e}")


def test_the_flat_limit_is_special_relativity():
    """A camera 1e6 M out: cos theta = (cos theta' - beta) / (1 - beta cos theta') about the velocity, and
    D_v = sqrt((1 + beta) / (1 - beta)) ahead, sqrt((1 - beta) / (1 + beta)) behind, to 1e-6."""
    for spin, axis in ((0.0, (0.0, 1.0, 0.0)), (0.9, (0.3, 1.0, -0.2))):
        hole = dc.Hole(BH, (spin, axis))
        ob = oc.Observer(hole, oc.moved_position(hole, (0.3, 1.4, 2.0), 1e6), BETA)
        b = math.sqrt(ob.b2)
        bh = np.array(BETA) / b
        npr = directions()
        d_eff, dv, dd = oc.observer_ray(ob, npr)
        ct_ = npr @ bh
        assert np.abs(d_eff @ bh - (ct_ - b) / (1.0 - b * ct_)).max() < 1e-6
        for s, want in ((1.0, math.sqrt((1 + b) / (1 - b))), (-1.0, math.sqrt((1 - b) / (1 + b)))):
            d1, dv1, dd1 = oc.observer_ray(ob, s * bh[None])
            assert abs(dv1[0] - want) < 1e-6 and abs(dd1[0] - want) < 1e-5 and np.abs(d1[0] - s * bh).max() < 1e-6


def test_the_inverse_velocity_undoes_the_aberration():
    """Applying -beta to n returns n' to 1e-14; |n| = 1 to 4 ulp."""
    for spin, r_m, hole, pos in pin_cases():
        ob = oc.Observer(hole, pos, BETA)
        back = oc.Observer(hole, pos, [-v for v in BETA])
        npr = directions()
        n, _ = oc.static_direction(ob, npr)
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
        n2, _ = oc.static_direction(back, n)
        assert np.abs(n2 - npr).max() < 1e-14


@pytest.mark.parametrize("r_m", [None, 40.0, 6.0])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_the_gpu_tests_velocity_moves_every_pixel(kerr, r_m):
    """The GPU tests' velocity, 0.4 c0 + 0.1 c1 - 0.2 c2 of the camera's axes, on the 96 x 72 frame of their
    camera (observer_check.observer_camera: 50 x 38.5 degrees; where it stands, 40 M and 6 M from the hole):
    d_eff departs from n' by more than 0.05 rad on at least 90 % of the pixels and D_v spans both sides of 1.
    (The 6-degree camera of tests/test_gpu_disk.py would not do: its D_v spans 1.08 .. 1.15 only.)"""
    hole = dc.Hole(BH, dc.KERRS[kerr])
    cam = oc.observer_camera(hole, r_m)
    npr = oc.pixel_directions(cam, W, H)
    for frame in (oc.STATIC, oc.COORDINATE):
        ob = oc.Observer(hole, list(cam.pos), oc.gpu_velocity(list(cam.c2w)), frame)
        d_eff, dv, dd = oc.observer_ray(ob, npr)
        ang = np.arccos(np.clip((d_eff * npr).sum(1), -1.0, 1.0))
        print(f"{kerr} {r_m} M {frame}: moved {100 * (ang > 0.05).mean():.1f} %, D_v {dv.min():.3f} .. {dv.max():.3f}, "
              f"D {dd.min():.3f} .. {dd.max():.3f}")
        assert (ang > 0.05).mean() >= 0.9
        assert dv.min() < 0.95 < 1.05 < dv.max()
