"""GPU: the pixel pass's separating half-space rule (rrt_proof.h rect_miss_proof, DESIGN.md §5;
launch constant KParams::halfspace, A/B knob RRT_AB_NO_HALFSPACE read at every launch).

Two 64 x 64 regions of the cfg3 frame at its full 1920 x 1080 framing and 64 spp -- tiles of 32 at
(896, 224) and at (1216, 640), where the rule proves most of what the slab test leaves (the numpy
mirror tests/rect_proof_sim.py on every second pixel: 317 -> 963 and 0 -> 722 of 1,024):

* RGB and counts through rrt_render_tiles_device, and RGB, counts and draws through rrt_render,
  equal the same render without the pixel pass (RRT_RENDER_NO_PIXEL_PROOF), the render with the
  rule off, and the region of the golden frame, bit for bit;
* a counting launch with the audit at every pixel re-marches every proven pixel and strip: no
  violation, and the rule adds at least half as many proven pixels as the mirror predicts.  The
  mirror runs on every second pixel each way, a quarter of the region's pixels on a regular grid,
  so its increase times 4 is the prediction for the region; device and mirror differ only in
  borderline pixels (the device contracts its arithmetic), far less than the factor 2 allows.
"""
import os

import numpy as np
import pytest

import rrt
from golden_cases import Case
from test_halfspace_proof import GPU_REGION_COUNTS

pytestmark = pytest.mark.gpu

CASE = "cfg3_bunny_1080p_s64"
REGIONS = sorted(GPU_REGION_COUNTS)
SIDE, TS = 64, 32
KNOB = "RRT_AB_NO_HALFSPACE"
COUNT_X = rrt.RRT_RENDER_COUNTERS | rrt.RRT_RENDER_COUNT_EXECUTED


class environ:
    """The knob's value for the launches inside (None: unset; the library reads it at every launch)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get(KNOB)
        if self.value is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.saved


@pytest.fixture(scope="module")
def gpu():
    c = Case(CASE)
    r = rrt.Renderer(device=0)
    r.set_scene(rrt.SceneFile(c.scene_path))
    r.set_envmap(c.envmap)
    r.set_camera(rrt.load_camera(c.camera_path))
    bh = c.cfg["bh"]
    r.set_black_hole(bh[:3], bh[3], bh[4])
    yield r
    r.close()


def params(c, flags=0):
    g = c.cfg
    return rrt.render_params(c.frame_w, c.frame_h, ns_aa=g["ns_aa"], max_ray_depth=g["max_ray_depth"],
                             ns_area_light=g["ns_area_light"], samples_per_batch=g["samples_per_batch"],
                             max_tolerance=g["max_tolerance"], direct_hemisphere=g["direct_hemisphere"], flags=flags)


def golden(c, x0, y0):
    sl = np.s_[y0 - c.y0:y0 - c.y0 + SIDE, x0 - c.x0:x0 - c.x0 + SIDE]
    return c.px["rgb"][sl], c.px["count"][sl], c.px["draws"][sl]


def tiles_render(gpu, p, x0, y0):
    """The region as four packed tiles of 32 through rrt_render_tiles_device -> rgb, count [64, 64]."""
    import torch
    tiles = np.array([(x0 + i * TS, y0 + j * TS) for j in range(2) for i in range(2)], np.uint32)
    prgb = torch.zeros(len(tiles) * TS * TS * 3, dtype=torch.float32, device="cuda")
    pcnt = torch.zeros(len(tiles) * TS * TS, dtype=torch.int32, device="cuda")
    gpu.render_tiles_device(p, tiles, TS, prgb.data_ptr(), pcnt.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rgb = prgb.cpu().numpy().reshape(2, 2, TS, TS, 3).transpose(0, 2, 1, 3, 4).reshape(SIDE, SIDE, 3)
    cnt = pcnt.cpu().numpy().reshape(2, 2, TS, TS).transpose(0, 2, 1, 3).reshape(SIDE, SIDE)
    return rgb, cnt


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("x0,y0", REGIONS)
def test_regions_are_the_same_bits(gpu, x0, y0):
    pytest.importorskip("torch")
    c = Case(CASE)
    ref = golden(c, x0, y0)
    for knob in (None, "1"):
        with environ(knob):
            on = gpu.render(params(c), x0, y0, SIDE, SIDE, draws=True)[:3]
            assert "rrt_batch_kernel<" in gpu.stats().kernel.decode()
            t_on = tiles_render(gpu, params(c), x0, y0)
            off = gpu.render(params(c, rrt.RRT_RENDER_NO_PIXEL_PROOF), x0, y0, SIDE, SIDE, draws=True)[:3]
            t_off = tiles_render(gpu, params(c, rrt.RRT_RENDER_NO_PIXEL_PROOF), x0, y0)
        assert same(on, off) and same(on, ref), (knob, x0, y0)
        assert same(t_on, t_off) and same(t_on, ref[:2]), (knob, x0, y0)


def audited(gpu, c, x0, y0, knob):
    """A counting launch of the region with every proven pixel and strip re-marched -> the tallies."""
    with environ(knob):
        gpu.proof_audit()  # reset
        gpu.set_proof_audit(0)
        rgb, cnt, _, _ = gpu.render(params(c, COUNT_X), x0, y0, SIDE, SIDE, counters=True)
        gpu.set_proof_audit(-1)
    ref = golden(c, x0, y0)
    assert same((rgb, cnt), ref[:2])
    return gpu.proof_audit()


def test_audit_no_violation_and_the_rule_fires(gpu):
    c = Case(CASE)
    # the audit tallies camera rays: a proven pixel's are the samples up to its first adaptive check
    n = min(c.cfg["ns_aa"], c.cfg["samples_per_batch"])
    for x0, y0 in REGIONS:
        t_on = audited(gpu, c, x0, y0, None)
        t_off = audited(gpu, c, x0, y0, "1")
        old, new = GPU_REGION_COUNTS[(x0, y0)]  # the mirror's, checked by tests/test_halfspace_proof.py
        print((x0, y0), "mirror, every second pixel:", old, "->", new, "device, every pixel: rays of proven pixels",
              t_off["pixel"]["checked"], "->", t_on["pixel"]["checked"], "of proven strips", t_off["strip"]["checked"],
              "->", t_on["strip"]["checked"], "at", n, "a pixel; violations", t_on["pixel"]["violations"],
              t_on["strip"]["violations"])
        for t in (t_on, t_off):
            assert t["pixel"]["violations"] == 0 and t["strip"]["violations"] == 0, t
            assert t["pixel"]["checked"] % n == 0 and t["strip"]["checked"] % n == 0, t
        assert t_on["pixel"]["checked"] > 0
        assert t_on["strip"]["checked"] >= t_off["strip"]["checked"]
        gain = (t_on["pixel"]["checked"] - t_off["pixel"]["checked"]) // n
        predicted = 4 * (new - old)
        assert predicted > 0
        assert 2 * gain >= predicted, (x0, y0, gain, predicted)
