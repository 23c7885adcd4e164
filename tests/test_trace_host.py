"""Host-side checks of the ray queries (rrt_trace_rays / rrt_trace_camera, include/rrt.h): the
exports and record sizes, the argument errors a host-only context can report, and the checker of
tests/trace_check.py pinned on the restatement alone."""
import ctypes as C
import os

import numpy as np
import pytest

import rrt
import trace_check as tc
from golden_cases import GOLD, Case

SPHERES = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
TRACE_SYMBOLS = ("rrt_trace_rays", "rrt_trace_rays_device", "rrt_trace_camera", "rrt_trace_camera_device")


def test_exports_and_record_sizes():
    L = rrt.lib()
    for name in TRACE_SYMBOLS:
        assert name in rrt.EXPORTS and hasattr(L, name), name
    assert rrt.RAY_DTYPE.itemsize == 48 and rrt.HIT_DTYPE.itemsize == 96
    assert C.sizeof(rrt.TraceParams) == 32
    # the record's tail: status, prim, bsdf, steps behind the ten doubles
    assert [rrt.HIT_DTYPE.fields[f][1] for f in ("hit_p", "n", "w_out", "t", "status", "prim", "bsdf", "steps")] == \
        [0, 24, 48, 72, 80, 84, 88, 92]
    assert L.rrt_abi_version() == 5  # additive: the ABI version stays


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


RAY = (np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, -1.0]]))


def test_no_scene_is_invalid(host):
    with pytest.raises(rrt.RRTError) as e:
        host.trace_rays(*RAY)
    assert e.value.code == rrt.RRT_E_INVALID
    with pytest.raises(rrt.RRTError) as e:
        host.trace_camera(8, 8, 0, 0, 8, 8)
    assert e.value.code == rrt.RRT_E_INVALID


def test_host_only_context_has_no_device(host):
    host.set_scene(rrt.SceneFile(SPHERES))
    for mode in ("auto", "lane", "wave"):
        for any_hit in (False, True):
            with pytest.raises(rrt.RRTError) as e:
                host.trace_rays(*RAY, any_hit=any_hit, mode=mode)
            assert e.value.code == rrt.RRT_E_NO_DEVICE
    host.set_camera(rrt.load_camera(Case("spheres_96x72_s1").camera_path))
    with pytest.raises(rrt.RRTError) as e:
        host.trace_camera(96, 72, 0, 0, 96, 72)
    assert e.value.code == rrt.RRT_E_NO_DEVICE


def test_camera_call_needs_a_camera(host):
    host.set_scene(rrt.SceneFile(SPHERES))
    with pytest.raises(rrt.RRTError) as e:
        host.trace_camera(96, 72, 0, 0, 96, 72)
    assert e.value.code == rrt.RRT_E_INVALID
    with pytest.raises(rrt.RRTError) as e:  # the ray call needs none: it gets as far as the device check
        host.trace_rays(*RAY)
    assert e.value.code == rrt.RRT_E_NO_DEVICE


def test_wave_mode_with_kerr_is_invalid(host):
    host.set_scene(rrt.SceneFile(SPHERES))
    host.set_black_hole(spin=0.9, axis=(0.3, 1.0, -0.2))
    with pytest.raises(rrt.RRTError) as e:
        host.trace_rays(*RAY, mode="wave")
    assert e.value.code == rrt.RRT_E_INVALID
    for mode in ("auto", "lane"):  # AUTO picks lane-per-ray there: valid, up to the device check
        with pytest.raises(rrt.RRTError) as e:
            host.trace_rays(*RAY, mode=mode)
        assert e.value.code == rrt.RRT_E_NO_DEVICE


def test_bad_params_and_regions_are_invalid(host):
    host.set_scene(rrt.SceneFile(SPHERES))
    host.set_camera(rrt.load_camera(Case("spheres_96x72_s1").camera_path))
    p = rrt.trace_params()
    p.mode = 3
    hits = np.zeros(1, rrt.HIT_DTYPE)
    assert rrt.lib().rrt_trace_camera(host.h, C.byref(p), 96, 72, 0, 0, 1, 1, hits.ctypes.data) == rrt.RRT_E_INVALID
    p = rrt.trace_params()
    p.flags = 2
    assert rrt.lib().rrt_trace_camera(host.h, C.byref(p), 96, 72, 0, 0, 1, 1, hits.ctypes.data) == rrt.RRT_E_INVALID
    with pytest.raises(rrt.RRTError) as e:  # region outside the frame
        host.trace_camera(96, 72, 90, 0, 17, 9)
    assert e.value.code == rrt.RRT_E_INVALID


def test_checker_self_test_on_the_restatement():
    """The single-primitive check is sound on the restatement alone: for every hit of one 256-ray
    set a brute-force search finds the (segment, primitive) pair reproducing ro_query's bits; the
    records built from it pass the checker, and damaged ones do not."""
    o, d = (a[:256] for a in tc.ray_sets()["interior"])
    orc = tc.Oracle(SPHERES)
    prims = tc.Prims(rrt.SceneFile(SPHERES))
    answers = orc.query(o, d)
    rec = tc.brute_force_records(orc, prims, o, d, answers)
    n_hit, n_cap, n_miss = tc.check_closest(orc, prims, o, d, answers, rec)
    assert n_hit >= 200 and n_hit + n_cap + n_miss == 256
    i = int(np.flatnonzero(rec["status"] == tc.HIT)[0])
    for field, value in (("steps", rec[i]["steps"] + 1), ("prim", (rec[i]["prim"] + 1) % len(prims)),
                         ("t", np.nextafter(rec[i]["t"], 1e9)), ("status", tc.MISS)):
        bad = rec.copy()
        bad[field][i] = value
        with pytest.raises(AssertionError):
            tc.check_closest(orc, prims, o, d, answers, bad)
    bad = rec.copy()
    bad["w_out"][i, 0] = -bad["w_out"][i, 0]
    with pytest.raises(AssertionError):
        tc.check_closest(orc, prims, o, d, answers, bad)
