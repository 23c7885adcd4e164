"""GPU: the LDS and scene accesses of the depth <= 1 kernels (and the path pool kernel's LDS slots)
after their address spaces are stated in the source: every pixel's RGB bits, sample
count and draw count against the CPU restatement (oracle/restate), on the settings that move the
LDS indexing and that the other small cases hold fixed:

  * frame 50x37 (the last tile clipped in both directions), default hole;
  * samples_per_batch 5, 8, 16, 32: groups of 8, 8, 16, 32 lanes, i.e. 32, 32, 16, 8 group records
    per 256-thread block (GroupLds), and the per-lane records (ShadeLds) shared accordingly;
  * ns_aa = 2 spb + 3: the last step is partial, so some lanes of a group idle;
  * the area-light batch build and the heavy pixels' kernel for every pixel (RRT_RENDER_HEAVY:
    HeavyLds, the out-of-line heavy_pixel_block);
  * spb 8 and 32 again on a point-light scene (build 2), with direct_hemisphere (general build) and
    with Kerr a/M 0.9 (the Kerr build);
  * one depth-3 frame through the path pool kernel (RRT_RENDER_WAVEFRONT: PathLds / OwnLds).

Bit-exact, no pixel left out: a load returns the same bytes whichever path carries it."""
import numpy as np
import pytest

import oracle_lib as ol
import rrt
from golden_cases import Case

pytestmark = pytest.mark.gpu

W, H = 50, 37
AREA = "spheres_96x72_s8_l4"    # CBspheres_lambertian: one area light (build 1)
POINT = "cfg4_knot_240x135_s16"  # point lights only (build 2)
KERR = (0.9, (0.0, 1.0, 0.0))
_oracle_cache = {}


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def settings(c, spb, **kw):
    g = c.cfg
    s = dict(ns_aa=2 * spb + 3, max_ray_depth=1, ns_area_light=g["ns_area_light"], samples_per_batch=spb,
             max_tolerance=g["max_tolerance"], direct_hemisphere=False)
    s.update(kw)
    return s


def oracle(c, w, h, s, kerr=None):
    key = (c.name, w, h, tuple(sorted(s.items())), kerr)
    if key not in _oracle_cache:
        p = ol.make_params(w, h, bh=c.cfg["bh"], kerr=kerr, **s)
        _oracle_cache[key] = ol.render(ol.Scene(c.scene_path), ol.load_camera(c.camera_path), p, 0, 0, w, h,
                                       threads=16)
    return _oracle_cache[key]


def render(gpu, c, w, h, s, flags=0, kerr=None):
    gpu.set_scene(rrt.SceneFile(c.scene_path))
    gpu.set_envmap(None)
    gpu.set_camera(rrt.load_camera(c.camera_path))
    bh = c.cfg["bh"]
    if kerr is None:
        gpu.set_black_hole(bh[:3], bh[3], bh[4])
    else:
        gpu.set_black_hole(bh[:3], bh[3], bh[4], spin=kerr[0], axis=kerr[1])
    return gpu.render(rrt.render_params(w, h, flags=flags, **s), 0, 0, w, h, draws=True)


def check(got, ref, what):
    rgb, cnt, draws, _ = got
    ref_rgb, ref_cnt, ref_draws, _ = ref
    bad = np.any(rgb.view(np.uint32) != ref_rgb.view(np.uint32), axis=-1) | (cnt != ref_cnt) | (draws != ref_draws)
    print(what, "pixels", bad.size, "differing", int(bad.sum()), "mean", float(rgb.mean()), "samples", int(cnt.sum()))
    assert float(ref_rgb.max()) > 0  # the frame renders something
    assert not bad.any(), (what, np.argwhere(bad)[:8].tolist())


@pytest.mark.parametrize("flags", [0, rrt.RRT_RENDER_HEAVY], ids=["batch", "heavy"])
@pytest.mark.parametrize("spb", [5, 8, 16, 32])
def test_group_sizes_area_light(gpu, spb, flags):
    c = Case(AREA)
    s = settings(c, spb)
    check(render(gpu, c, W, H, s, flags=flags), oracle(c, W, H, s), f"area spb {spb} flags {flags:#x}")


@pytest.mark.parametrize("spb", [8, 32])
def test_group_sizes_point_light(gpu, spb):
    c = Case(POINT)
    s = settings(c, spb)
    check(render(gpu, c, W, H, s), oracle(c, W, H, s), f"point spb {spb}")


@pytest.mark.parametrize("spb", [8, 32])
def test_group_sizes_hemisphere(gpu, spb):
    c = Case(AREA)
    s = settings(c, spb, direct_hemisphere=True)
    check(render(gpu, c, W, H, s), oracle(c, W, H, s), f"hemisphere spb {spb}")


@pytest.mark.parametrize("spb", [8, 32])
def test_group_sizes_kerr(gpu, spb):
    c = Case(AREA)
    s = settings(c, spb)
    check(render(gpu, c, W, H, s, kerr=KERR), oracle(c, W, H, s, kerr=KERR), f"kerr spb {spb}")
    gpu.set_black_hole(c.cfg["bh"][:3], c.cfg["bh"][3], c.cfg["bh"][4])


def test_path_pool_depth3(gpu):
    c = Case(AREA)
    s = settings(c, 8, max_ray_depth=3)
    check(render(gpu, c, W, H, s, flags=rrt.RRT_RENDER_WAVEFRONT), oracle(c, W, H, s), "path pool depth 3")
