"""CPU: the exit rules of DESIGN.md §11 pinned on the restatement alone -- the numpy stepper of
tests/exit_check.py against ro_micro_chain bit for bit, the Schwarzschild rule in the flat limit,
the Kerr rule against the weak-field deflection -- and the argument checks a host-only context can
make for RRT_TRACE_EXIT and rrt_env_eval."""
import ctypes as C
import os

import numpy as np
import pytest

import exit_check as xc
import oracle_lib as ol
import rrt
import trace_check as tc
from golden_cases import GOLD

SPHERES = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
HOLES = {"default": tc.DEFAULT_BH, "flat": (0.0, 1.0, 0.0, 0.0, 0.1), "dt0.5": (0.0, 1.0, 0.0, 0.1, 0.5),
         "dt0.04": (0.0, 1.0, 0.0, 0.1, 0.04), "moved": (0.3, 0.6, -0.2, 0.25, 0.1)}
O, D = (a[:300] for a in tc.ray_sets()["interior"])


@pytest.mark.parametrize("hole", sorted(HOLES))
def test_numpy_stepper_reproduces_the_chain_bit_for_bit(hole):
    bh = HOLES[hole]
    ch = xc.Chains(bh, O, D)
    assert ch.rows == tc.steps_of(bh[4])
    ok = 0
    for i in range(len(O)):
        out = np.zeros((ch.rows, 8))
        n = ol.lib().ro_micro_chain(np.array(bh, np.float64), O[i].copy(), D[i].copy(), out, ch.rows)
        assert n >= 1
        ok += tc.same(ch.seg[:n, i, :], out[:n, :7])
    print(f"{hole}: {ok} / {len(O)} chains bit-identical, escape rows {ch.jstar.min()}..{ch.jstar.max()}, "
          f"escaped {int(ch.escaped.sum())}")
    assert ok == len(O)


@pytest.mark.parametrize("dt,bound", [(0.1, 2e-5), (0.04, 2e-6), (0.5, 3e-3)])
def test_flat_limit_exit_direction_is_the_ray(dt, bound):
    """r_s = 0: the geodesic is the straight ray, so the exit direction is the ray's own up to the
    stepper's error (~dtheta^4)."""
    ch = xc.Chains((0.0, 1.0, 0.0, 0.0, dt), O, D)
    assert ch.escaped.all() and (ch.jstar < ch.rows).all()
    a = xc.angle(ch.e, D)
    print(f"dtheta {dt}: largest angle between e and d {a.max():.3g} rad (bound {bound:g})")
    assert a.max() <= bound
    assert np.abs(np.linalg.norm(ch.e, axis=-1) - 1.0).max() < 1e-12


@pytest.mark.parametrize("b_over_m", [50.0, 100.0])
def test_kerr_exit_chord_shows_the_weak_field_deflection(b_over_m):
    """a = 0, M = 0.05, dtheta = 0.1: a ray from 1000 M out, in the equatorial plane, along +x with
    impact parameter b leaves along its exit row's chord, deflected by 4 M / b + 15 pi M^2 / (4 b^2)
    to within 1% (the third-order term (128 / 3)(M / b)^3 accounts for the rest)."""
    M = 0.05
    bh = (0.0, 1.0, 0.0, 2.0 * M, 0.1)
    b = b_over_m * M
    o = np.array([-np.sqrt((1000.0 * M) ** 2 - b * b), 1.0, b])
    d = np.array([1.0, 0.0, 0.0])
    ch, _ = ol.kerr_chain(bh, 0.0, (0.0, 1.0, 0.0), o, d, max_rows=600)
    q2 = (ch[:, 8] * ch[:, 8] + ch[:, 9] * ch[:, 9]) + ch[:, 10] * ch[:, 10]
    assert not ch[:, 7].any() and q2[0] < xc.kerr_far2(bh)
    K = int(np.argmax(q2 > xc.kerr_far2(bh)))
    assert K > 0 and q2[K] > xc.kerr_far2(bh)
    got = float(xc.angle(ch[K, 3:6][None], d[None])[0])
    want = 4.0 * M / b + 15.0 * np.pi * M * M / (4.0 * b * b)
    print(f"b = {b_over_m} M: exit row {K}, deflection {got:.6g} rad, series {want:.6g} ({(got / want - 1) * 100:+.2f}%)")
    assert abs(got / want - 1.0) <= 0.01


@pytest.fixture()
def host():
    r = rrt.Renderer(device=-1)
    yield r
    r.close()


RAY = (np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, -1.0]]))


def test_exit_flag_reaches_the_device_check(host):
    assert rrt.lib().rrt_abi_version() == 5
    assert (rrt.RRT_TRACE_EXIT, rrt.RRT_RAY_ESCAPED, rrt.RRT_SPACETIME_LENSED_SKY) == (4, 3, 1)
    host.set_scene(rrt.SceneFile(SPHERES))
    for kw in ({}, {"spin": 0.9}):
        host.set_black_hole(lensed_sky=True, **kw)
        for mode in ("auto", "lane") + (() if kw else ("wave",)):
            for any_hit in (False, True):
                with pytest.raises(rrt.RRTError) as e:
                    host.trace_rays(*RAY, any_hit=any_hit, mode=mode, exit=True)
                assert e.value.code == rrt.RRT_E_NO_DEVICE
    with pytest.raises(rrt.RRTError) as e:  # Kerr has no wave-per-ray kernel, flagged or not
        host.trace_rays(*RAY, mode="wave", exit=True)
    assert e.value.code == rrt.RRT_E_INVALID
    hits = np.zeros(1, rrt.HIT_DTYPE)
    rays = np.zeros(1, rrt.RAY_DTYPE)
    for flags, want in ((2, rrt.RRT_E_INVALID), (2 | 4, rrt.RRT_E_INVALID), (8, rrt.RRT_E_INVALID), (4 | 1, rrt.RRT_E_NO_DEVICE)):
        p = rrt.trace_params()
        p.flags = flags
        assert rrt.lib().rrt_trace_rays(host.h, C.byref(p), rays.ctypes.data, 1, hits.ctypes.data) == want, flags


def test_env_eval_arguments(host):
    assert "rrt_env_eval" in rrt.EXPORTS and hasattr(rrt.lib(), "rrt_env_eval")
    with pytest.raises(rrt.RRTError) as e:
        host.env_eval(np.array([[0.0, 1.0, 0.0]]))
    assert e.value.code == rrt.RRT_E_INVALID
    host.set_envmap(np.ones((4, 8, 3), np.float32))
    with pytest.raises(rrt.RRTError) as e:
        host.env_eval(np.array([[0.0, 1.0, 0.0]]))
    assert e.value.code == rrt.RRT_E_NO_DEVICE
    host.set_envmap(None)
    with pytest.raises(rrt.RRTError) as e:
        host.env_eval(np.array([[0.0, 1.0, 0.0]]))
    assert e.value.code == rrt.RRT_E_INVALID
