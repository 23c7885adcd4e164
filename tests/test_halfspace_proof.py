"""The pixel pass's separating half-space rule (rrt_proof.h rect_miss_proof; numpy
mirror tests/rect_proof_sim.py) against the CPU restatement of the reference's march (oracle
ro_camera_ray / ro_micro_chain), on random pixels and 8 x 8 strips of the BASELINE framings:

* soundness: every ray of a rectangle the mirror proves -- its four corners and random jitters --
  misses: none of its reference segments reaches the root box (test_pixel_proof's loose slab test);
* superset: whatever tests/pixel_proof_sim.py proves the new mirror proves, and with the rule off
  the two agree;
* gain: on cfg3 and cfg2 the rule raises the proven share of the sampled pixels by at least 0.04
  (measured on 3,600-pixel grids of the frames: +0.069 and +0.059), which fails if it never fires.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import pixel_proof_sim
import rect_proof_sim
import rrt
from golden_cases import Case
from miss_proof_sim import constants
from test_pixel_proof import _loose_root_hit

# (case, least gain of the proven share over the old mirror's on the same pixels)
CASES = [("cfg1_spheres_480x360_s8", None), ("cfg2_spheres_1080p_s64_flat", 0.04), ("cfg3_bunny_1080p_s64", 0.04),
         ("cfg4_knot_4k_s256_crop", None)]
N_PIX = 600
N_JIT = 6
N_STRIPS = 60
# The two 64 x 64 regions of the cfg3 frame that tests/test_gpu_halfspace_proof.py renders: (x0, y0) ->
# proven pixels (old mirror, new mirror) among every second pixel each way (1,024 a region).  The GPU
# test sets the device's count against these; test_gpu_region_counts below keeps them the mirror's.
GPU_REGION_COUNTS = {(896, 224): (317, 963), (1216, 640): (0, 722)}


@functools.lru_cache(maxsize=None)
def _framing(name):
    c = Case(name)
    bh = np.array(c.cfg["bh"], np.float64)
    r = rrt.Renderer(device=-1)
    r.set_scene(rrt.SceneFile(c.scene_path))
    boxes, _, _ = r.bvh()
    r.close()
    lo, hi = boxes[0][:3].copy(), boxes[0][3:].copy()
    K = constants(bh, lo, hi)
    cam = O.load_camera(c.camera_path)
    cols = np.array(cam.c2w, np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(cam.pos, np.float64)
    W, H = c.frame_w, c.frame_h
    mn, mx = C.c_double(), C.c_double()

    def ray(sx, sy):
        o, d = np.zeros(3), np.zeros(3)
        O.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, sx / W, sy / H, o, d,
                              C.byref(mn), C.byref(mx))
        return o, d

    return bh, K, lo, hi, W, H, ray


def _three_proofs(K, o, dc, corners):
    """(old mirror, new mirror with the rule off, new mirror); the first two must agree and the
    third may only add."""
    old = pixel_proof_sim.prove(K, o, dc, corners)
    off = rect_proof_sim.prove(K, o, dc, corners, halfspace=False)
    new = rect_proof_sim.prove(K, o, dc, corners)
    assert off == old
    assert new or not old
    return old, new


def _assert_rays_miss(name, bh, K, lo, hi, ray, out, pts):
    for sx, sy in pts:
        o2, d2 = ray(sx, sy)
        k = O.lib().ro_micro_chain(bh, o2, d2, out, K["steps"] + 1)
        assert not _loose_root_hit(lo, hi, out[:k]).any(), (name, sx, sy)


@pytest.mark.parametrize("name,min_gain", CASES)
def test_halfspace_pixels(name, min_gain):
    bh, K, lo, hi, W, H, ray = _framing(name)
    g = np.random.default_rng(5)
    pxs = g.integers(0, W, N_PIX)
    pys = g.integers(0, H, N_PIX)
    out = np.zeros((K["steps"] + 1, 8))
    n_old = n_new = 0
    for px, py in zip(pxs, pys):
        o, dc = ray(px + 0.5, py + 0.5)
        corners = np.array([ray(px + (k & 1), py + (k >> 1))[1] for k in range(4)])
        old, new = _three_proofs(K, o, dc, corners)
        n_old += old
        n_new += new
        if not new:
            continue
        jit = [(float(k & 1), float(k >> 1)) for k in range(4)] + [tuple(g.random(2)) for _ in range(N_JIT)]
        _assert_rays_miss(name, bh, K, lo, hi, ray, out, [(px + jx, py + jy) for jx, jy in jit])
    print(name, "proven pixels: old mirror", n_old / N_PIX, "with the half-space rule", n_new / N_PIX)
    if min_gain is not None:
        assert n_new / N_PIX - n_old / N_PIX >= min_gain


@pytest.mark.parametrize("x0,y0", sorted(GPU_REGION_COUNTS))
def test_gpu_region_counts(x0, y0):
    _, K, _, _, _, _, ray = _framing("cfg3_bunny_1080p_s64")
    n_old = n_new = 0
    for py in range(y0, y0 + 64, 2):
        for px in range(x0, x0 + 64, 2):
            o, dc = ray(px + 0.5, py + 0.5)
            corners = np.array([ray(px + (k & 1), py + (k >> 1))[1] for k in range(4)])
            new = rect_proof_sim.prove(K, o, dc, corners)
            n_new += new
            n_old += new and pixel_proof_sim.prove(K, o, dc, corners)  # a subset: test_halfspace_pixels
    assert (n_old, n_new) == GPU_REGION_COUNTS[(x0, y0)]


@pytest.mark.parametrize("name", ["cfg3_bunny_1080p_s64", "cfg4_knot_4k_s256_crop"])
def test_halfspace_strips(name):
    """8 x 8 strips (the pass's strip level): the four corners and six jitters of a proven strip
    miss, and so does every pixel of it, at two corners and a random jitter each."""
    bh, K, lo, hi, W, H, ray = _framing(name)
    g = np.random.default_rng(9)
    out = np.zeros((K["steps"] + 1, 8))
    n_old = n_new = 0
    for _ in range(N_STRIPS):
        x0 = int(g.integers(0, W - 7)) // 8 * 8
        y0 = int(g.integers(0, H - 7)) // 8 * 8
        o, dc = ray(x0 + 4.0, y0 + 4.0)
        corners = np.array([ray(x0 + (k & 1) * 8, y0 + (k >> 1) * 8)[1] for k in range(4)])
        old, new = _three_proofs(K, o, dc, corners)
        n_old += old
        n_new += new
        if not new:
            continue
        pts = [(x0 + 8.0 * (k & 1), y0 + 8.0 * (k >> 1)) for k in range(4)]
        pts += [(x0 + 8.0 * jx, y0 + 8.0 * jy) for jx, jy in g.random((N_JIT, 2))]
        for j in range(8):
            for i in range(8):
                pts += [(x0 + i + jx, y0 + j + jy) for jx, jy in [(0.0, 0.0), (1.0, 1.0), tuple(g.random(2))]]
        _assert_rays_miss(name, bh, K, lo, hi, ray, out, pts)
    print(name, "proven strips: old mirror", n_old / N_STRIPS, "with the half-space rule", n_new / N_STRIPS)
