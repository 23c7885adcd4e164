"""GPU: the launch constants are scoped to the stage that uses them (launch constants by
stage): the batch and heavy kernels read a KParams field again, through the scalar path, where a stage
starts.  One Renderer, never recreated, goes twice through a sequence of launches whose constants all
differ -- three holes on the area-light build, the point-light build, another mesh, a crop of a larger
frame -- and every frame must equal its golden bit for bit (RGB, sample counts, draw counts).  A
constant left over from the previous launch, or a field re-read through the scalar path that a kernel
of the launch writes, shows up here.

One more launch takes the heavy and continuation path, which reads records written during the launch:
a crop (<= 60 % of the frame) of the point-light scene with continuations forced on.  The golden's
settings (16 samples, checks every 32) can hand no pixel over -- a continuation needs three adaptive
steps -- so this launch checks every 5 samples and is compared with the CPU restatement (oracle/restate)."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import rrt
from golden_cases import Case

pytestmark = pytest.mark.gpu

# (case, crop (x, y, w, h) of its golden or None)
SEQUENCE = [("bunny_160x120_s16", None), ("bunny_B1_160x120_s16", None), ("bunny_B3_160x120_s16", None),
            ("cfg4_knot_240x135_s16", None), ("banana_64x48_s16", None), ("cfg1_spheres_480x360_s8", (208, 156, 64, 48))]
CONT_ENV = {"RRT_AB_CONT": "1", "RRT_AB_CONT_MIN": "1", "RRT_AB_CONT_ROOM": "64"}


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


def test_sequence_of_launches_twice(gpu):
    kernels = set()
    for rnd in range(2):
        for name, crop in SEQUENCE:
            c = Case(name)
            x, y, w, h = crop if crop else (c.x0, c.y0, c.w, c.h)
            setup(gpu, c)
            rgb, cnt, draws, _ = gpu.render(rrt.render_params(c.frame_w, c.frame_h, **settings(c)), x, y, w, h, draws=True)
            kernels.add(gpu.stats().kernel.decode())
            ys, xs = slice(y - c.y0, y - c.y0 + h), slice(x - c.x0, x - c.x0 + w)
            ref_rgb, ref_cnt, ref_draws = c.px["rgb"][ys, xs], c.px["count"][ys, xs], c.px["draws"][ys, xs]
            bad = np.any(rgb.view(np.uint32) != ref_rgb.view(np.uint32), axis=-1) | (cnt != ref_cnt) | (draws != ref_draws)
            print("round", rnd, name, "pixels", bad.size, "differing", int(bad.sum()), "samples", int(cnt.sum()))
            assert float(ref_rgb.max()) > 0  # the frame renders something
            assert not bad.any(), (rnd, name, np.argwhere(bad)[:8].tolist())
    print(sorted(kernels))
    # the area-light and the point-light batch builds both ran
    assert any("rrt_batch_kernel<1," in k for k in kernels) and any("rrt_batch_kernel<2," in k for k in kernels)


def test_continuations_on_a_crop(gpu):
    c = Case("cfg4_knot_240x135_s16")
    x, y, w, h = 72, 32, 96, 72  # <= 60 % of the frame: the heavy list and continuations run
    s = settings(c, samples_per_batch=5)
    p = ol.make_params(c.frame_w, c.frame_h, bh=c.cfg["bh"], **s)
    ref_rgb, ref_cnt, ref_draws, _ = ol.render(ol.Scene(c.scene_path), ol.load_camera(c.camera_path), p, x, y, w, h, threads=16)
    saved = {k: os.environ.get(k) for k in CONT_ENV}
    os.environ.update(CONT_ENV)  # read by the library at every launch
    try:
        setup(gpu, c)
        rgb, cnt, draws, _ = gpu.render(rrt.render_params(c.frame_w, c.frame_h, **s), x, y, w, h, draws=True)
        st = gpu.stats()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    bad = np.any(rgb.view(np.uint32) != ref_rgb.view(np.uint32), axis=-1) | (cnt != ref_cnt) | (draws != ref_draws)
    print("continuations", st.last_cont_pixels, "heavy", st.last_heavy_pixels, st.kernel.decode(), "differing", int(bad.sum()))
    assert float(ref_rgb.max()) > 0
    assert st.last_cont_pixels > 0  # some pixel goes past its first check and is handed over
    assert not bad.any(), np.argwhere(bad)[:8].tolist()
