"""GPU parity of the ray queries (rrt_trace_rays / rrt_trace_camera, csrc/rrt_query.hip): every
field of every record against the CPU restatement, by the exact checker of tests/trace_check.py;
lane-per-ray and wave-per-ray records byte-identical; sizes around a wave and a block with guard
records; camera rays; and the render path untouched by a trace on the same context."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import rrt
import trace_check as tc
from golden_cases import GOLD, Case

pytestmark = pytest.mark.gpu

SCENES = {"spheres": os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts"),
          "bunny": os.path.join(GOLD, "scenes", "CBbunny.rrts")}
# (scene, ray set): each set on CBspheres_lambertian, and (O, R) on CBbunny
SETS = [("spheres", "interior"), ("spheres", "aimed"), ("spheres", "outward"), ("spheres", "inward"),
        ("bunny", "interior")]
# Schwarzschild holes (cx, cy, cz, r_s, dtheta): dtheta 0.04 is 158 steps (a second round of the
# wave mode), 0.5 is 13 (fewer than a wave); a moved hole; r_s = 0 (the flat limit)
HOLES = {"default": tc.DEFAULT_BH, "dt0.04": (0.0, 1.0, 0.0, 0.1, 0.04), "dt0.5": (0.0, 1.0, 0.0, 0.1, 0.5),
         "moved": (0.3, 0.6, -0.2, 0.25, 0.1), "flat": (0.0, 1.0, 0.0, 0.0, 0.1)}
KERRS = {"a0.9": (0.9, (0.3, 1.0, -0.2)), "a0": (0.0, (0.0, 1.0, 0.0))}
# what the restatement must show on CBspheres_lambertian with the default hole before anything is
# compared: (hits, captured, misses) at least
MIN_COUNTS = {"interior": (400, 0, 0), "aimed": (0, 256, 0), "outward": (64, 0, 128), "inward": (256, 0, 32)}

RAYS = tc.ray_sets()
_prims, _oracles = {}, {}


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def prims_of(scene):
    if scene not in _prims:
        _prims[scene] = tc.Prims(rrt.SceneFile(SCENES[scene]))
    return _prims[scene]


def oracle_of(scene, rset, bh, kerr=None):
    """(Oracle, its answers for the ray set), computed once and left unchanged."""
    key = (scene, rset, bh, kerr)
    if key not in _oracles:
        orc = tc.Oracle(SCENES[scene], bh, kerr)
        _oracles[key] = (orc, orc.query(*RAYS[rset]))
    return _oracles[key]


def setup(gpu, scene, bh, kerr=None):
    gpu.set_scene(rrt.SceneFile(SCENES[scene]))
    if kerr is None:
        gpu.set_black_hole(bh[:3], bh[3], bh[4])
    else:
        gpu.set_black_hole(bh[:3], bh[3], bh[4], spin=kerr[0], axis=kerr[1])


@pytest.mark.parametrize("hole", sorted(HOLES))
@pytest.mark.parametrize("scene,rset", SETS)
def test_parity_schwarzschild(gpu, scene, rset, hole):
    bh = HOLES[hole]
    o, d = RAYS[rset]
    orc, answers = oracle_of(scene, rset, bh)
    if scene == "spheres" and hole == "default":
        seen = tc.restatement_counts(orc, o, d, answers)
        assert all(c >= m for c, m in zip(seen, MIN_COUNTS[rset])), seen
    setup(gpu, scene, bh)
    lane = gpu.trace_rays(o, d, mode="lane")
    counts = tc.check_closest(orc, prims_of(scene), o, d, answers, lane)
    print(f"{scene}/{rset}/{hole}: hit / captured / miss = {counts}, max steps {lane['steps'].max()}")
    wave = gpu.trace_rays(o, d, mode="wave")
    assert lane.tobytes() == wave.tobytes()
    auto = gpu.trace_rays(o, d)
    assert lane.tobytes() == auto.tobytes()
    lane_any = gpu.trace_rays(o, d, any_hit=True, mode="lane")
    tc.check_any(lane, lane_any)
    assert lane_any.tobytes() == gpu.trace_rays(o, d, any_hit=True, mode="wave").tobytes()


@pytest.mark.parametrize("kerr", sorted(KERRS))
@pytest.mark.parametrize("scene,rset", SETS)
def test_parity_kerr(gpu, scene, rset, kerr):
    o, d = RAYS[rset]
    orc, answers = oracle_of(scene, rset, tc.DEFAULT_BH, KERRS[kerr])
    setup(gpu, scene, tc.DEFAULT_BH, KERRS[kerr])
    lane = gpu.trace_rays(o, d, mode="lane")
    counts = tc.check_closest(orc, prims_of(scene), o, d, answers, lane)
    print(f"{scene}/{rset}/kerr {kerr}: hit / captured / miss = {counts}, max steps {lane['steps'].max()}")
    assert lane.tobytes() == gpu.trace_rays(o, d).tobytes()  # AUTO picks lane-per-ray
    tc.check_any(lane, gpu.trace_rays(o, d, any_hit=True, mode="lane"))
    with pytest.raises(rrt.RRTError) as e:
        gpu.trace_rays(o, d, mode="wave")
    assert e.value.code == rrt.RRT_E_INVALID


@pytest.mark.parametrize("mode", ["lane", "wave"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes_and_guard_records(gpu, n, mode):
    """The device entry point on a buffer of n + 64 records pre-filled with 0xA5: the first n are the
    rays' records, the 64 guard records stay untouched."""
    import torch
    o, d = (a[:n] for a in RAYS["interior"])
    orc, answers = oracle_of("spheres", "interior", tc.DEFAULT_BH)
    setup(gpu, "spheres", tc.DEFAULT_BH)
    rays = np.zeros(max(n, 1), rrt.RAY_DTYPE)
    rays["o"][:n], rays["d"][:n] = o, d
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.full(((n + 64) * 96,), 0xA5, dtype=torch.uint8, device="cuda")
    gpu.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), mode=mode,
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_hits.cpu().numpy()
    assert (out[n * 96:] == 0xA5).all()
    tc.check_closest(orc, prims_of("spheres"), o, d, answers[:n], out[:n * 96].view(rrt.HIT_DTYPE))


def camera_rays(c, xs, ys):
    cam = ol.load_camera(c.camera_path)
    cols = np.array(cam.c2w, np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(cam.pos, np.float64)
    o, d = np.zeros((len(xs), 3)), np.zeros((len(xs), 3))
    mn, mx = C.c_double(), C.c_double()
    for i, (x, y) in enumerate(zip(xs, ys)):
        ol.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, (x + 0.5) / c.frame_w,
                               (y + 0.5) / c.frame_h, o[i], d[i], C.byref(mn), C.byref(mx))
    return o, d


@pytest.mark.parametrize("name,kerr", [("spheres_96x72_s1", None), ("bunny_160x120_s16", (0.9, (0.3, 1.0, -0.2)))])
def test_camera(gpu, name, kerr):
    """trace_camera over the whole frame and a 17 x 9 region at (5, 3): every third pixel of the
    frame (both ways) against ro_camera_ray + the restatement's query; the region equals the frame there."""
    c = Case(name)
    bh = tc.DEFAULT_BH
    setup(gpu, "spheres" if "spheres" in name else "bunny", bh, kerr)
    gpu.set_camera(rrt.load_camera(c.camera_path))
    modes = ["lane"] if kerr else ["lane", "wave"]
    frame = gpu.trace_camera(c.frame_w, c.frame_h, 0, 0, c.frame_w, c.frame_h, mode="lane")
    assert frame.shape == (c.frame_h, c.frame_w)
    xs, ys = (a.ravel() for a in np.meshgrid(np.arange(0, c.frame_w, 3), np.arange(0, c.frame_h, 3)))
    o, d = camera_rays(c, xs, ys)
    orc = tc.Oracle(c.scene_path, bh, kerr)
    counts = tc.check_closest(orc, tc.Prims(rrt.SceneFile(c.scene_path)), o, d, orc.query(o, d), frame[ys, xs])
    print(f"{name}: hit / captured / miss = {counts}")
    # the spheres frame shows 707 hits and 61 captures on the restatement; the lensed bunny frame hits
    assert counts[0] >= (600 if kerr is None else 100) and (kerr is not None or counts[1] >= 40), counts
    for mode in modes:
        region = gpu.trace_camera(c.frame_w, c.frame_h, 5, 3, 17, 9, mode=mode)
        assert region.tobytes() == np.ascontiguousarray(frame[3:12, 5:22]).tobytes()
        tc.check_any(frame, gpu.trace_camera(c.frame_w, c.frame_h, 0, 0, c.frame_w, c.frame_h, any_hit=True, mode=mode))
    assert frame.tobytes() == gpu.trace_camera(c.frame_w, c.frame_h, 0, 0, c.frame_w, c.frame_h).tobytes()


def test_render_after_trace_is_unchanged_and_fenced(gpu):
    """After trace calls the smoke render (spheres_96x72_s1, 4 spp) on the same context is still
    bit-exact; a trace on a stream other than the previous render's is ordered after it (the
    workspace fence): its records are the checked ones, and the render's output is complete."""
    import torch
    c = Case("spheres_96x72_s1")
    gpu.set_scene(rrt.SceneFile(c.scene_path))
    gpu.set_camera(rrt.load_camera(c.camera_path))
    gpu.set_black_hole()
    o, d = RAYS["interior"]
    want = gpu.trace_rays(o, d, mode="lane")
    gpu.trace_camera(c.frame_w, c.frame_h, 0, 0, c.frame_w, c.frame_h)
    p = rrt.render_params(c.frame_w, c.frame_h, ns_aa=4)
    rgb, cnt, draws, _ = gpu.render(p, 0, 0, c.frame_w, c.frame_h, draws=True)
    orgb, ocnt, odraws, _ = ol.render(ol.Scene(c.scene_path), ol.load_camera(c.camera_path),
                                      ol.make_params(c.frame_w, c.frame_h, ns_aa=4), 0, 0, c.frame_w, c.frame_h, threads=16)
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32))
    assert np.array_equal(cnt, ocnt) and np.array_equal(draws, odraws)
    # render on stream A (device buffers), trace on stream B without any host wait in between
    tiles = rrt.partition_tiles(c.frame_w, c.frame_h, 32, 0, 1)  # [nt, 2]
    nt = len(tiles)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_rgb = torch.zeros(nt * 32 * 32 * 3, dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(nt * 32 * 32, dtype=torch.int32, device="cuda")
    rays = np.zeros(len(o), rrt.RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(len(o) * 96, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu.render_tiles_device(p, tiles, 32, d_rgb.data_ptr(), d_cnt.data_ptr(), stream=sa.cuda_stream)
    gpu.trace_rays_device(d_rays.data_ptr(), len(o), d_hits.data_ptr(), mode="wave", stream=sb.cuda_stream)
    torch.cuda.synchronize()
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    got = d_rgb.cpu().numpy().reshape(nt, 32, 32, 3)
    cn = d_cnt.cpu().numpy().reshape(nt, 32, 32)
    for t in range(nt):
        x0, y0 = int(tiles[t, 0]), int(tiles[t, 1])
        w, h = min(32, c.frame_w - x0), min(32, c.frame_h - y0)
        assert np.array_equal(got[t, :h, :w].view(np.uint32), orgb[y0:y0 + h, x0:x0 + w].view(np.uint32))
        assert np.array_equal(cn[t, :h, :w], ocnt[y0:y0 + h, x0:x0 + w])
