"""GPU: the camera miss proof gate (DESIGN.md §5 "Proof gate").  The area- and point-light batch
kernels run the per-ray miss proof only in front of rays their group expects to miss
(RRT_AB_PROVE_FIRST=0, the default); RRT_AB_PROVE_FIRST=1, read at every launch, proves every ray
first, as before the gate.  The proof is a shortcut ("proven => the exact march returns no hit"), so
both settings must give the reference's frame bit for bit: RGB, sample counts and draw counts.

Cases: a whole small frame with box-silhouette pixels of both hints and the hole; a hole off the
scene's centre; the point-light build; lit 64-sample pixels (a second step whose hypothesis comes
from the first step's last sample).

The `lost` re-query (a hit whose record a lane gave up and the chain then landed on, rrt_batch_kernel)
now marches without the proof.  With area lights a hit takes more draw-offset slots than a miss, so
in a group whose lanes are all busy a mostly-hit pixel with one miss gives up the records of the
hits beyond it (the lanes holding them take the unknown slots), and a second miss shifts the chain
back onto such a slot.  RESTATED["lost"] renders the bunny's silhouette and the hole that way --
8-sample steps on 8 lanes -- and RESTATED["cont"] is the forced-continuation launch of
tests/test_gpu_launch_constants.py, whose heavy kernel takes listed and handed-over pixels; both are
compared with the CPU restatement (oracle/restate), as there.  That the re-query round itself runs
in RESTATED["lost"] rests on the argument above, not on a count: the kernel keeps no tally of it
outside the profile build, so the test asserts only what the restatement can show, that the frame
holds pixels with both outcomes (95 of them) on the area-light build."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import rrt
from golden_cases import Case

pytestmark = pytest.mark.gpu

KNOB = "RRT_AB_PROVE_FIRST"
ALWAYS, BY_HYPOTHESIS = "1", "0"
CASES = ["bunny_160x120_s16", "spheres_bh_96x72_s8", "cfg4_knot_240x135_s16", "bunny_1080p_s64_crop"]
CONT_ENV = {"RRT_AB_CONT": "1", "RRT_AB_CONT_MIN": "1", "RRT_AB_CONT_ROOM": "64"}


class environ:
    """The environment values for the launches inside (the library reads them at every launch)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def setup(gpu, c):
    gpu.set_scene(rrt.SceneFile(c.scene_path))
    gpu.set_envmap(c.envmap)
    gpu.set_camera(rrt.load_camera(c.camera_path))
    bh = c.cfg["bh"]
    gpu.set_black_hole(bh[:3], bh[3], bh[4])


def settings(c, **kw):
    g = c.cfg
    s = dict(ns_aa=g["ns_aa"], max_ray_depth=g["max_ray_depth"], ns_area_light=g["ns_area_light"],
             samples_per_batch=g["samples_per_batch"], max_tolerance=g["max_tolerance"],
             direct_hemisphere=g["direct_hemisphere"])
    s.update(kw)
    return s


def differing(got, ref):
    (rgb, cnt, draws), (ref_rgb, ref_cnt, ref_draws) = got, ref
    return np.any(rgb.view(np.uint32) != ref_rgb.view(np.uint32), axis=-1) | (cnt != ref_cnt) | (draws != ref_draws)


def render_golden(gpu, c, knob, flags=0):
    """The case's golden region at the knob's value (None: unset) -> the pixels that differ from the golden."""
    setup(gpu, c)
    with environ(**{KNOB: knob}):
        rgb, cnt, draws, _ = gpu.render(rrt.render_params(c.frame_w, c.frame_h, flags=flags, **settings(c)),
                                        c.x0, c.y0, c.w, c.h, draws=True)
    return differing((rgb, cnt, draws), (c.px["rgb"], c.px["count"], c.px["draws"]))


@pytest.mark.parametrize("knob", [ALWAYS, BY_HYPOTHESIS, None], ids=["always", "by_hypothesis", "default"])
@pytest.mark.parametrize("name", CASES)
def test_frame_equals_golden(gpu, name, knob):
    bad = render_golden(gpu, Case(name), knob)
    print(name, knob, gpu.stats().kernel.decode(), "pixels", bad.size, "differing", int(bad.sum()))
    assert "rrt_batch_kernel<" in gpu.stats().kernel.decode()
    assert not bad.any(), np.argwhere(bad)[:8].tolist()


# launches compared with the CPU restatement: (case, crop (x, y, w, h), settings, environment)
#  cont: tests/test_gpu_launch_constants.py's forced continuations (point lights: a hit and a miss take
#        the same draws, so no slot is ever off the chain; the heavy kernel takes both kinds of pixel)
#  lost: area lights, 8-sample steps on 8 busy lanes across the bunny's silhouette and the hole
RESTATED = {
    "cont": ("cfg4_knot_240x135_s16", (72, 32, 96, 72), dict(samples_per_batch=5), CONT_ENV),
    "lost": ("bunny_160x120_s16", (0, 0, 160, 120), dict(samples_per_batch=8), {}),
}
_restated = {}


def restated(tag):
    """(case, crop, settings, environment, the restatement's rgb / count / draws), computed once."""
    if tag not in _restated:
        name, (x, y, w, h), kw, env = RESTATED[tag]
        c = Case(name)
        s = settings(c, **kw)
        p = ol.make_params(c.frame_w, c.frame_h, bh=c.cfg["bh"], **s)
        ref = ol.render(ol.Scene(c.scene_path), ol.load_camera(c.camera_path), p, x, y, w, h, threads=16)[:3]
        _restated[tag] = (c, (x, y, w, h), s, env, ref)
    return _restated[tag]


@pytest.mark.parametrize("knob", [ALWAYS, BY_HYPOTHESIS], ids=["always", "by_hypothesis"])
@pytest.mark.parametrize("tag", sorted(RESTATED))
def test_mixed_steps_equal_the_restatement(gpu, tag, knob):
    c, (x, y, w, h), s, env, ref = restated(tag)
    setup(gpu, c)
    with environ(**env, **{KNOB: knob}):
        rgb, cnt, draws, _ = gpu.render(rrt.render_params(c.frame_w, c.frame_h, **s), x, y, w, h, draws=True)
        st = gpu.stats()
    bad = differing((rgb, cnt, draws), ref)
    # a pixel with hits and misses: its draws lie strictly between all-miss (2 a sample) and all-hit
    hi = int((ref[2] // np.maximum(ref[1], 1)).max())
    mixed = (ref[2] > 2 * ref[1]) & (ref[2] < hi * ref[1])
    print(tag, knob, "continuations", st.last_cont_pixels, "heavy", st.last_heavy_pixels, st.kernel.decode(),
          "draws per sample up to", hi, "mixed pixels", int(mixed.sum()), "differing", int(bad.sum()))
    assert float(ref[0].max()) > 0
    if tag == "cont":  # the heavy kernel ran, and some pixel went past its first check and was handed over
        assert st.last_heavy_pixels > 0 and st.last_cont_pixels > 0
    else:
        assert "rrt_batch_kernel<1," in st.kernel.decode() and hi > 2 and mixed.sum() > 50
    assert not bad.any(), np.argwhere(bad)[:8].tolist()


def test_knob_is_read_at_every_launch(gpu):
    """Two values on one Renderer, back to back and back again: the plan reads the environment anew."""
    c = Case("bunny_160x120_s16")
    for knob in (ALWAYS, BY_HYPOTHESIS, ALWAYS):
        with environ(**{KNOB: knob}):
            assert rrt.lib().rrt_plan_prove_first() == int(knob)
        bad = render_golden(gpu, c, knob)
        assert not bad.any(), (knob, np.argwhere(bad)[:8].tolist())


@pytest.mark.parametrize("knob", [ALWAYS, BY_HYPOTHESIS], ids=["always", "by_hypothesis"])
def test_no_miss_proof_launch_is_unaffected(gpu, knob):
    bad = render_golden(gpu, Case("bunny_160x120_s16"), knob, flags=rrt.RRT_RENDER_NO_MISS_PROOF)
    assert not bad.any(), np.argwhere(bad)[:8].tolist()
