#!/usr/bin/env python3
"""Measurement of the ray queries (rrt_trace_camera_device, csrc/rrt_query.hip) on the cfg3 framing
(CBbunny, 1920x1080, Schwarzschild r_s 0.1, dtheta 0.1), one process:

* time per call of the lane-per-ray and wave-per-ray modes at n = 1, 64, 4096 and 2^20 pixel-centre
  rays (square regions about the frame's centre; 256, 1024 and 3025 too, to place the crossing), the
  two modes alternated call by call, next to what AUTO picks there;
* the full-frame trace against rrt_render_tiles_device of the same frame at ns_aa 1, max_ray_depth 0
  with the miss proof, the pixel proof and the heavy path off -- existing code doing the same one
  exact camera query per pixel, plus shading -- alternated call by call.

Every call is timed by device events on the current stream around the call, followed by a
synchronise; each variant is warmed up first.  Writes a JSON record (with the library's build_id).
Usage: python3 tools/trace_bench.py --out profiles/trace_rays.json"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: one shared HIP runtime)
import bench  # noqa: E402
import rrt  # noqa: E402


def timed(fn):
    """Milliseconds between device events around one call, after a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "calls": len(ms)}


def alternate(variants, reps, warmup=2):
    """{name: summary} of callables timed in turn, reps rounds, each warmed up first."""
    for fn in variants.values():
        for _ in range(warmup):
            timed(fn)
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn))
    return {k: summary(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frame-reps", type=int, default=10)
    a = ap.parse_args()
    wl = bench.WORKLOADS["cfg3"]
    W, H = wl["w"], wl["h"]
    r = rrt.Renderer(0)
    scene, cam, _, _ = bench.load_workload_scene(wl, tempfile.mkdtemp(prefix="rrt_tb_"))
    r.set_scene(scene)
    r.set_camera(rrt.camera_desc(cam))
    r.set_black_hole(*wl["bh"])
    s = torch.cuda.current_stream().cuda_stream
    hits = torch.zeros(W * H * 96, dtype=torch.uint8, device="cuda")
    res = {"build_id": rrt.build_id(), "device": torch.cuda.get_device_name(0), "workload": wl["desc"],
           "timing": "device events around each call on one stream, then a synchronise; variants alternated",
           "modes": {}, "frame": {}}

    # n = 1, 64, 4096, 2^20, and 256, 1024, 3025 between them to place the crossing
    for side in (1, 8, 16, 32, 55, 64, 1024):
        w, h = side, side
        x0, y0 = (W - w) // 2, (H - h) // 2
        n = w * h

        def call(mode, x0=x0, y0=y0, w=w, h=h):
            return lambda: r.trace_camera_device(W, H, x0, y0, w, h, hits.data_ptr(), mode=mode, stream=s)

        reps = a.reps if n < (1 << 20) else max(3, a.reps // 4)
        t = alternate({"lane": call("lane"), "wave": call("wave"), "auto": call("auto")}, reps)
        # the modes' records are identical: checked here at the sizes timed
        out = {}
        for mode in ("lane", "wave"):
            hits.zero_()
            call(mode)()
            torch.cuda.synchronize()
            out[mode] = hits[:n * 96].clone()
        t["identical_records"] = bool(torch.equal(out["lane"], out["wave"]))
        res["modes"][str(n)] = t
        print(n, json.dumps(t), flush=True)

    # the comparison owed: full-frame trace against the depth-0, 1-spp render with every ray marched
    ts = 32
    tiles = rrt.partition_tiles(W, H, ts, 0, 1)
    nt = len(tiles)
    prgb = torch.zeros(nt * ts * ts * 3, dtype=torch.float32, device="cuda")
    pcnt = torch.zeros(nt * ts * ts, dtype=torch.int32, device="cuda")
    flags = rrt.RRT_RENDER_NO_MISS_PROOF | rrt.RRT_RENDER_NO_PIXEL_PROOF | rrt.RRT_RENDER_NO_HEAVY
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0, flags=flags)
    t = alternate({
        "render_1spp_depth0_exact": lambda: r.render_tiles_device(p, tiles, ts, prgb.data_ptr(), pcnt.data_ptr(), stream=s),
        "trace_camera_lane": lambda: r.trace_camera_device(W, H, 0, 0, W, H, hits.data_ptr(), mode="lane", stream=s),
        "trace_camera_any_lane": lambda: r.trace_camera_device(W, H, 0, 0, W, H, hits.data_ptr(), any_hit=True,
                                                              mode="lane", stream=s),
    }, a.frame_reps)
    t["render_kernel"] = r.stats().kernel.decode()
    res["frame"] = t
    print("frame", json.dumps(t), flush=True)
    r.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
