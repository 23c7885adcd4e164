"""GPU: the shadow-ray occlusion proof's re-entry rule (rrt_proof.h occ_exit; launch
constant KParams::shadow_reentry, A/B knob RRT_AB_NO_SHADOW_REENTRY read at every launch).

The two smallest framings that hold shadow rays which leave the room past the hole and come back
through a wall: the whole bunny_160x120_s16 frame, and the 64 x 64 region at (1024, 576) of the cfg3
frame at its full 1920 x 1080 framing and 64 spp (in the numpy mirror tests/shadow_reentry_sim.py about
half of that region's shadow rays are newly proven).  For each:

* a counting launch with the audit at every proven ray (every one is re-marched exactly), rule off
  and on: the frame equals the golden bit for bit, no shadow violation, and the rule proves at least
  1.2 x as many shadow rays (the mirror gives 1.42 x on the first framing and more on the second; the
  margin is for the difference between the mirror's ray set and the render's);
* a plain render gives the golden's bits at both knob values.
"""
import os

import numpy as np
import pytest

import rrt
from golden_cases import Case

pytestmark = pytest.mark.gpu

KNOB = "RRT_AB_NO_SHADOW_REENTRY"
COUNT_X = rrt.RRT_RENDER_COUNTERS | rrt.RRT_RENDER_COUNT_EXECUTED
# case, region (x0, y0, w, h; None: the whole frame)
FRAMINGS = [("bunny_160x120_s16", None), ("cfg3_bunny_1080p_s64", (1024, 576, 64, 64))]


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


@pytest.fixture(scope="module", params=FRAMINGS, ids=[f[0] for f in FRAMINGS])
def framing(request):
    name, region = request.param
    c = Case(name)
    r = rrt.Renderer(device=0)
    r.set_scene(rrt.SceneFile(c.scene_path))
    r.set_envmap(c.envmap)
    r.set_camera(rrt.load_camera(c.camera_path))
    bh = c.cfg["bh"]
    r.set_black_hole(bh[:3], bh[3], bh[4])
    yield r, c, region or (c.x0, c.y0, c.w, c.h)
    r.close()


def params(c, flags=0):
    g = c.cfg
    return rrt.render_params(c.frame_w, c.frame_h, ns_aa=g["ns_aa"], max_ray_depth=g["max_ray_depth"],
                             ns_area_light=g["ns_area_light"], samples_per_batch=g["samples_per_batch"],
                             max_tolerance=g["max_tolerance"], direct_hemisphere=g["direct_hemisphere"], flags=flags)


def golden(c, region):
    x0, y0, w, h = region
    sl = np.s_[y0 - c.y0:y0 - c.y0 + h, x0 - c.x0:x0 - c.x0 + w]
    return c.px["rgb"][sl], c.px["count"][sl], c.px["draws"][sl]


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def audited(gpu, c, region, knob):
    """A counting launch of the region with every proven ray re-marched -> the tallies."""
    with environ(knob):
        gpu.proof_audit()  # reset
        gpu.set_proof_audit(0)
        rgb, cnt, _, _ = gpu.render(params(c, COUNT_X), *region, counters=True)
        gpu.set_proof_audit(-1)
    assert same((rgb, cnt), golden(c, region)[:2]), knob
    return gpu.proof_audit()


def test_audit_no_violation_and_the_rule_proves_more(framing):
    gpu, c, region = framing
    t_off = audited(gpu, c, region, "1")
    t_on = audited(gpu, c, region, None)
    print(c.name, region, "shadow rays proven and re-marched:", t_off["shadow"]["checked"], "->", t_on["shadow"]["checked"],
          "violations", t_off["shadow"]["violations"], t_on["shadow"]["violations"])
    assert t_off["shadow"]["violations"] == 0 and t_on["shadow"]["violations"] == 0
    assert t_off["shadow"]["checked"] > 0
    assert 10 * t_on["shadow"]["checked"] >= 12 * t_off["shadow"]["checked"]


def test_plain_render_is_the_same_bits(framing):
    gpu, c, region = framing
    ref = golden(c, region)
    for knob in (None, "1"):
        with environ(knob):
            got = gpu.render(params(c), *region, draws=True)[:3]
        assert same(got, ref), knob
