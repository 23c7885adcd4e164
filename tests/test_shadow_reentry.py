"""The shadow-ray occlusion proof's re-entry rule (rrt_proof.h occ_exit, KParams::shadow_reentry;
DESIGN.md §5; numpy mirror tests/shadow_reentry_sim.py) against the CPU restatement of the
reference's march (oracle ro_micro_chain / ro_tri_intersect / ro_shadow_query).

A segment end that has left the root box without a certain crossing no longer ends the proof: the
recurrence goes on under the same per-row conditions, and a later segment that certainly crosses a
kept wall triangle proves "occluded".  Checked on

* the shadow rays a render casts: one jittered camera ray per pixel of a grid of the frame, its
  closest hit (ro_query), a uniform point of the area light, rays that start below the surface
  dropped -- cfg3 every 12th pixel, bunny_160x120_s16 every 2nd, cfg1 every 6th;
* tests/test_shadow_proof.py's surface-to-light rays, from the ray itself (lead 0) and from the
  reference's state after two exact segments (lead 2);
* a small sweep of random configurations inside the proofs' envelope (tests/proof_sweep.py
  draw_config).

Every proven ray: the reference's chain is uncaptured through the proof's segment, the reference's
triangle test accepts that segment against the proof's triangle, and the reference's shadow query
returns true.  The recurrence stays within 1e-3 of the margin of the reference's points on every row
the proof ran, the rows after leaving included.  Every ray the old rule proves is proven at the same
row and triangle.  The share proven on the camera-visible sets is at least three points under the
measured 0.96 / 0.935 / 0.964.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import proof_sweep
import rrt
from golden_cases import Case
from miss_proof_sim import constants
from shadow_proof_sim import occluders, run as run_old, trigger_box
from shadow_reentry_sim import check_config, compare, run
from test_shadow_proof import CASES, N, _shadow_rays

VISIBLE = [("cfg3_bunny_1080p_s64", 12, 0.93), ("bunny_160x120_s16", 2, 0.90), ("cfg1_spheres_480x360_s8", 6, 0.93)]
EPS = 1e-11


@functools.lru_cache(maxsize=None)
def _scene(name):
    c = Case(name)
    sf = rrt.SceneFile(c.scene_path)
    sc = O.Scene(c.scene_path)
    boxes, _, _ = sc.bvh()
    lo, hi = boxes[0][:3].copy(), boxes[0][3:].copy()
    T = sf.triangles()
    faces, w = occluders(T, lo, hi)
    bh = np.array(c.cfg["bh"], np.float64)
    K = constants(bh, lo, hi)
    p = O.make_params(c.frame_w, c.frame_h, ns_aa=c.cfg["ns_aa"], bh=tuple(bh))
    return c, sf, sc, T, faces, trigger_box(K, w), bh, K, p


def _visible_rays(name, stride, seed=3):
    """The shadow rays of one jittered camera ray per pixel of every stride-th row and column."""
    c, sf, sc, _, _, _, _, _, p = _scene(name)
    cam = O.load_camera(c.camera_path)
    cols = np.array(cam.c2w, np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(cam.pos, np.float64)
    ls = [lv for ty, _, lv in sf.lights() if ty in (0, 1)]
    kinds = [ty for ty, _, _ in sf.lights() if ty in (0, 1)]
    g = np.random.default_rng(seed)
    mn, mx = C.c_double(), C.c_double()
    os_, ds = [], []
    for y in range(stride // 2, c.frame_h, stride):
        for x in range(stride // 2, c.frame_w, stride):
            o, d = np.zeros(3), np.zeros(3)
            O.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, (x + g.random()) / c.frame_w,
                                  (y + g.random()) / c.frame_h, o, d, C.byref(mn), C.byref(mx))
            hit, hp, n, _ = O.query(sc, p, o, d)
            if not hit:
                continue
            k = g.integers(0, len(ls))
            lv = ls[k]
            pt = lv[0] + ((g.random() - 0.5) * lv[2] + (g.random() - 0.5) * lv[3] if kinds[k] == 0 else 0.0)
            wi = pt - hp
            wi /= np.linalg.norm(wi)
            if wi @ (n / np.linalg.norm(n)) < 0:  # the light is below the surface: no shadow ray
                continue
            os_.append(hp + EPS * wi)
            ds.append(wi)
    return np.array(os_), np.array(ds)


def _check(tag, r, sc, p, o0, d0):
    """compare()'s result r on rays whose render-side rays are (o0, d0): the assertions every set shares."""
    print(tag, "rays", r["rays"], "proven", r["proven_before"], "->", r["proven_after"], "after leaving",
          r["proven_after_leaving"], "rows after leaving", np.bincount(r["rows_after_leaving"] or [0]).tolist(),
          "worst deviation / margin", r["worst_dev_over_margin"], "violations", r["violations"], "lost", r["lost"])
    assert r["worst_dev_over_margin"] < 1e-3
    assert not r["violations"]
    assert not r["lost"]
    untrue = [int(i) for i in np.nonzero(r["proven"])[0] if not O.shadow_query(sc, p, o0[i], d0[i])]
    assert not untrue, untrue


@pytest.mark.parametrize("name,stride,min_share", VISIBLE)
def test_camera_visible_shadow_rays(name, stride, min_share):
    _, _, sc, T, faces, box, bh, K, p = _scene(name)
    o, d = _visible_rays(name, stride)
    rows, nrow = proof_sweep._chains(bh, o, d, K["steps"])
    r = compare(K, faces, box, T, o, d, rows, nrow)
    _check((name, stride), r, sc, p, o, d)
    assert r["proven_after"] / r["rays"] >= min_share
    assert r["proven_after_leaving"] > 0


@functools.lru_cache(maxsize=None)
def _surface_set(name):
    _, sf, _, T, _, _, bh, K, _ = _scene(name)
    o, d = _shadow_rays(T, sf.lights(), N, 11)
    rows, nrow = proof_sweep._chains(bh, o, d, K["steps"])
    return o, d, rows, nrow


@pytest.mark.parametrize("lead", [0, 2])
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_surface_to_light_rays(name, lead):
    """lead: the exact segments marched before the proof takes over from the reference's state."""
    _, _, sc, T, faces, box, _, K, p = _scene(name)
    o0, d0, rows, nrow = _surface_set(name)
    o, d = o0, d0
    if lead:  # rays whose first `lead` reference segments neither hit a wall nor were captured
        keep = (nrow > lead) & ~rows[:, :lead, 7].any(1)
        o, d = rows[keep, lead, 0:3].copy(), rows[keep, lead - 1, 3:6].copy()
        rows, nrow, o0, d0 = rows[keep][:, lead:], nrow[keep] - lead, o0[keep], d0[keep]
    r = compare(dict(K, steps=K["steps"] - lead), faces, box, T, o, d, rows, nrow)
    _check((name, lead), r, sc, p, o0, d0)
    assert r["proven_after"] >= r["proven_before"]


def test_mirror_without_the_rule_is_the_old_mirror():
    """run(reentry=False) and tests/shadow_proof_sim.py run give the same arrays, NaNs included."""
    _, _, _, _, faces, box, _, K, _ = _scene("bunny_160x120_s16")
    o, d = _visible_rays("bunny_160x120_s16", 2)
    old = run_old(K, faces, box, o, d)
    new = run(K, faces, box, o, d, reentry=False)
    for a, b in zip(old, new[:5]):
        np.testing.assert_array_equal(a, b)
    assert ((new[5] >= 0) <= ~new[0]).all()  # a ray that left was not proven


def test_envelope_sweep():
    g = np.random.default_rng(21)
    for i in range(6):
        cfg = proof_sweep.draw_config(g)
        r = check_config(cfg, 300, g)
        print(i, cfg["scene"], [round(float(v), 3) for v in cfg["bh"]], r)
        assert r["violations"] == 0 and r["lost"] == 0
        assert r["worst_dev_over_margin"] < 1e-3
