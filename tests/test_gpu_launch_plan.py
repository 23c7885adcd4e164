"""The launch record of rrt_render / rrt_render_tiles_device (rrt_host.cpp: check_launch, plan_launch,
enqueue): for each call of ROWS the kernel name, the grid, the heavy-list and continuation capacities
the launch got (rrt_get_stats) and the sha256 of the frame's rgb, count and draws bytes; for a refused
call its error code and message.  tests/golden/launch_plan.json holds the records of the library
before the launch path was split into its stages; every field must come out the same.

grid_blocks depends on the device's CU count: the fixture stores the recording device's, and the
grid is compared only on a device with as many.

Recording (once, with the library to pin selected through RRT_LIB):
    RRT_LIB=/path/to/librrt.so python tests/test_gpu_launch_plan.py
runs every row twice on fresh contexts and leaves out (and names) a row whose two records differ."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # (under pytest, conftest.py has done both)
    try:
        import torch  # noqa: F401  (first: one shared HIP runtime)
    except Exception:
        pass
    sys.path.insert(0, os.path.join(HERE, "..", "relativistic-ray-tracer_amd"))

import disk_check as dc
import rrt
from golden_cases import GOLD, Case
from test_gpu_address_spaces import AREA, KERR, POINT, settings

FIXTURE = os.path.join(GOLD, "launch_plan.json")
W, H = 50, 37  # the last tile clipped both ways
PART = dict(frame=(96, 72), region=(32, 32, 32, 32))  # under 60% of the frame: heavy pixels on by share
ENV_KEYS = ("RRT_AB_CONT", "RRT_AB_CONT_MIN", "RRT_AB_CONT_ROOM", "RRT_AB_CONT_WAITERS")
EM = (2.0, 1.0, 0.5)
DISK_KERR = dc.KERRS["a0.9"]
F = rrt


def row(scene=AREA, spb=8, flags=0, variant=0, kerr=None, sky=False, disk=None, frame=(W, H), region=None, env=None,
        counters=False, tiles=None, **s):
    """One call: settings(case, spb, **s) of tests/test_gpu_address_spaces.py on `scene`; kerr (spin,
    axis); sky: the lensed sky; disk: set_disk keywords; env: RRT_AB_* for the call; tiles: a tile size,
    for a call through render_tiles_device with one tile."""
    return dict(scene=scene, spb=spb, flags=flags, variant=variant, kerr=kerr, sky=sky, disk=disk, frame=frame,
                region=region or (0, 0) + tuple(frame), env=env or {}, counters=counters, tiles=tiles, s=s)


def disk(**kw):
    return dict(r_in=0.0, r_out=dc.R_OUT, emission=EM, **kw)


ROWS = {
    # the batch family, area lights (build 1)
    "area": row(),
    "area_one_queue": row(flags=F.RRT_RENDER_ONE_QUEUE),
    "area_xcd_queues": row(flags=F.RRT_RENDER_XCD_QUEUES),
    "area_striped_queues": row(flags=F.RRT_RENDER_STRIPED_QUEUES),
    "area_ordered": row(flags=F.RRT_RENDER_ORDERED),
    "area_prepass": row(flags=F.RRT_RENDER_PREPASS),
    "area_no_pixel_proof": row(flags=F.RRT_RENDER_NO_PIXEL_PROOF),
    "area_heavy": row(flags=F.RRT_RENDER_HEAVY),
    "area_no_heavy": row(flags=F.RRT_RENDER_NO_HEAVY),
    "area_waves2": row(variant=2),
    "area_waves3": row(variant=3),
    "area_waves5": row(variant=5),
    # point lights (build 2), direct_hemisphere (build 0), Kerr
    "point": row(scene=POINT),
    "point_waves3": row(scene=POINT, variant=3),
    "hemisphere": row(direct_hemisphere=True),
    "hemisphere_one_queue": row(direct_hemisphere=True, flags=F.RRT_RENDER_ONE_QUEUE),
    "kerr": row(kerr=KERR),
    # a part of the frame
    "part": row(**PART),
    "part_s64": row(ns_aa=64, **PART),
    "part_s64_cont1": row(ns_aa=64, env={"RRT_AB_CONT": "1"}, **PART),
    "part_s64_cont0": row(ns_aa=64, env={"RRT_AB_CONT": "0"}, **PART),
    "part_s64_eager": row(ns_aa=64, env={"RRT_AB_CONT": "1", "RRT_AB_CONT_MIN": "1", "RRT_AB_CONT_ROOM": "64"}, **PART),
    # depth >= 2
    "deep3": row(max_ray_depth=3),
    "deep3_no_pixel_proof": row(max_ray_depth=3, flags=F.RRT_RENDER_NO_PIXEL_PROOF),
    "deep3_sample": row(max_ray_depth=3, flags=F.RRT_RENDER_DEEP_SAMPLE),
    "deep3_sample_waves2": row(max_ray_depth=3, flags=F.RRT_RENDER_DEEP_SAMPLE, variant=2),
    "deep3_sample_waves4": row(max_ray_depth=3, flags=F.RRT_RENDER_DEEP_SAMPLE, variant=4),
    "deep3_path_pool": row(max_ray_depth=3, flags=F.RRT_RENDER_WAVEFRONT),
    "deep3_path_pool_waves2": row(max_ray_depth=3, flags=F.RRT_RENDER_WAVEFRONT, variant=2),
    "deep3_path_pool_waves4": row(max_ray_depth=3, flags=F.RRT_RENDER_WAVEFRONT, variant=4),
    "deep5": row(max_ray_depth=5),
    # a switch flag, the lensed sky, the disk builds
    "thin_lens": row(flags=F.RRT_RENDER_THIN_LENS),
    "sky": row(sky=True),
    "sky_kerr": row(sky=True, kerr=KERR),
    "disk": row(kerr=DISK_KERR, disk=disk()),
    "disk_bb": row(kerr=DISK_KERR, disk=disk(temperature=6000.0)),
    "disk_light": row(kerr=DISK_KERR, disk=disk(light=True)),
    "disk_bb_light": row(kerr=DISK_KERR, disk=disk(temperature=6000.0, light=True)),
    "disk_pt": row(kerr=DISK_KERR, disk=disk(temperature=6000.0, profile="page-thorne")),
    "disk_pt_light": row(kerr=DISK_KERR, disk=disk(temperature=6000.0, profile="page-thorne", light=True)),
    # refused
    "no_switch_with_kerr": row(kerr=KERR, flags=F.RRT_RENDER_THIN_LENS),
    "no_illum3_depth0": row(flags=F.RRT_RENDER_ILLUM(3), max_ray_depth=0),
    "no_sky_path_pool": row(sky=True, max_ray_depth=3, flags=F.RRT_RENDER_WAVEFRONT),
    "no_disk_counters": row(kerr=DISK_KERR, disk=disk(), counters=True),
    "no_path_pool_depth1": row(flags=F.RRT_RENDER_WAVEFRONT),
    "no_tile_size_12": row(tiles=12),
    "no_spb_0": row(samples_per_batch=0),
    "no_depth_17": row(max_ray_depth=17),
    "no_disk_schwarzschild": row(disk=disk()),
    "no_sky_path_pool_switch": row(sky=True, max_ray_depth=3, flags=F.RRT_RENDER_WAVEFRONT | F.RRT_RENDER_THIN_LENS),
}
# the per-sample family, the per-pixel flags and the counting kernels, on both metrics
for _tag, _kerr in (("", None), ("_kerr", KERR)):
    ROWS["sample_s4" + _tag] = row(ns_aa=4, kerr=_kerr)
    ROWS["per_pixel" + _tag] = row(flags=F.RRT_RENDER_PER_PIXEL, kerr=_kerr)
    ROWS["pixel_loop" + _tag] = row(flags=F.RRT_RENDER_PIXEL_LOOP, kerr=_kerr)
    ROWS["counters" + _tag] = row(counters=True, kerr=_kerr)
    ROWS["counters_executed" + _tag] = row(counters=True, flags=F.RRT_RENDER_COUNT_EXECUTED, kerr=_kerr)

# a host-only context (device=-1): what it holds, and the call (either entry point; no pointer is read)
HOST_ROWS = {f"{what}_{via}": dict(what=what, via=via)
             for what in ("no_scene", "no_camera", "bad_disk", "valid") for via in ("render", "tiles")}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def refusal(e):
    return {"error": e.code, "message": str(e).split(": ", 1)[1]}


def run_row(gpu, r):
    c = Case(r["scene"])
    bh = c.cfg["bh"]
    gpu.set_scene(rrt.SceneFile(c.scene_path))
    gpu.set_envmap(Case("env_bunny_96x72_s16").envmap if r["sky"] else None)
    gpu.set_camera(rrt.load_camera(c.camera_path))
    k = r["kerr"]
    gpu.set_black_hole(bh[:3], bh[3], bh[4], lensed_sky=r["sky"], **({} if k is None else dict(spin=k[0], axis=k[1])))
    if r["disk"] is None:
        gpu.set_disk(None)
    else:
        gpu.set_disk(**r["disk"])
    (fw, fh), (x0, y0, w, h) = r["frame"], r["region"]
    p = rrt.render_params(fw, fh, flags=r["flags"], variant=r["variant"], **settings(c, r["spb"], **r["s"]))
    saved = {key: os.environ.pop(key, None) for key in ENV_KEYS}
    os.environ.update(r["env"])
    try:
        if r["tiles"]:
            import torch
            ts = r["tiles"]
            rgb = torch.zeros(ts * ts * 3, dtype=torch.float32, device="cuda")
            cnt = torch.zeros(ts * ts, dtype=torch.int32, device="cuda")
            gpu.render_tiles_device(p, np.zeros((1, 2), np.uint32), ts, rgb.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            rgb, cnt, draws = rgb.cpu().numpy(), cnt.cpu().numpy(), np.zeros(0, np.uint32)
        else:
            rgb, cnt, draws, _ = gpu.render(p, x0, y0, w, h, draws=True, counters=r["counters"])
    except rrt.RRTError as e:
        return refusal(e)
    finally:
        for key in ENV_KEYS:
            os.environ.pop(key, None)
        os.environ.update({key: v for key, v in saved.items() if v is not None})
        gpu.set_disk(None)
    st = gpu.stats()
    return {"kernel": st.kernel.decode(), "grid_blocks": st.grid_blocks, "last_heavy_pixels": st.last_heavy_pixels,
            "last_cont_pixels": st.last_cont_pixels, "rgb": sha(rgb), "count": sha(cnt), "draws": sha(draws)}


def run_host_row(r):
    host = rrt.Renderer(device=-1)
    try:
        c = Case(AREA)
        if r["what"] != "no_scene":
            host.set_scene(rrt.SceneFile(c.scene_path))
        if r["what"] not in ("no_scene", "no_camera"):
            host.set_camera(rrt.load_camera(c.camera_path))
        if r["what"] == "bad_disk":  # r_in below the ISCO of a/M = 0 (6 M)
            host.set_black_hole(c.cfg["bh"][:3], c.cfg["bh"][3], c.cfg["bh"][4], spin=0.0)
            host.set_disk(2.0, dc.R_OUT)
        p = rrt.render_params(W, H, **settings(c, 8))
        try:
            if r["via"] == "render":
                host.render(p, 0, 0, W, H)
            else:
                host.render_tiles_device(p, np.zeros((1, 2), np.uint32), 32, 16, 16)
        except rrt.RRTError as e:
            return refusal(e)
        return {"error": 0, "message": ""}
    finally:
        host.close()


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_launch_record(gpu, golden, name):
    want = dict(golden["rows"][name])
    got = run_row(gpu, ROWS[name])
    print(name, got)
    if golden["cu_count"] != cu_count():
        want.pop("grid_blocks", None)
        got.pop("grid_blocks", None)
    assert got == want


@pytest.mark.parametrize("name", sorted(HOST_ROWS))
def test_host_only_refusals(golden, name):
    got = run_host_row(HOST_ROWS[name])
    print(name, got)
    assert got["error"] != 0
    assert got == golden["host_rows"][name]


if __name__ == "__main__":
    runs = []
    for _ in range(2):
        g = rrt.Renderer(device=0)
        runs.append({n: run_row(g, ROWS[n]) for n in sorted(ROWS)})
        g.close()
    unstable = sorted(n for n in ROWS if runs[0][n] != runs[1][n])
    for n in unstable:
        print("not reproducible, left out:", n, runs[0][n], runs[1][n])
    out = {"cu_count": cu_count(), "library": rrt.build_id(),
           "rows": {n: v for n, v in runs[0].items() if n not in unstable},
           "host_rows": {n: run_host_row(HOST_ROWS[n]) for n in sorted(HOST_ROWS)}}
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for n in sorted(out["rows"]):
        print(n, out["rows"][n])
    print("wrote", path, "rows", len(out["rows"]), "left out", unstable)
