"""GPU: the opt-in builds of the general per-pixel-loop kernel at depth >= 1 -- the lensed sky (V_SKY 5,
V_KERR_SKY 6), the accretion disk (V_KERR_DISK 7; §12) and the disk light
(V_KERR_DISK_LIGHT 9; §14) -- whole frames against the CPU restatement (oracle/restate ro_render_events)
bit for bit: RGB, sample counts and RNG draws, with jittered camera rays, the adaptive sample loop
(samples_per_batch 4), listed-light and environment shadow rays, hemisphere sampling, bounces off
diffuse, mirror and glass surfaces, and the disk light's draws after the listed lights'.

The restatement's new code is pinned against the independent numpy checkers by
tests/test_disk_oracle.py.  Its per-pixel event counts prove that a frame holds the cases it claims to
hold: each case names floors on the number of pixels in which an event happened at all.  The floors
are conditions on the case, not measurements of the kernel: they are evaluated on the restatement's
counts alone.

Frames are 96 x 72 of CBspheres / CBspheres_lambertian through the wide camera
(cfg1_spheres_480x360_s8's) with the default hole as Kerr (tests/disk_check.py KERRS), or 64 x 48 of
banana_64x48_s16 with the lensed frame's hole of tests/test_gpu_lensed_sky.py."""
import os

import numpy as np
import pytest

import disk_check as dc
import oracle_lib as ol
import rrt
import trace_check as tc
from golden_cases import GOLD, Case
from test_gpu_lensed_sky import FRAME_BH, FRAME_KERR

pytestmark = pytest.mark.gpu
W, H = 96, 72
WIDE_CASE = "cfg1_spheres_480x360_s8"
BANANA = "banana_64x48_s16"
EM = (20.0, 10.0, 5.0)
THREADS = 16
_frames = {}


def room(build, scene, kerr, r_out, depth, ns_aa, nal, floors, hemi=False, lensed=False, redshift=True, light=False):
    return dict(build=build, scene=os.path.join(GOLD, "scenes", scene + ".rrts"), camera=Case(WIDE_CASE).camera_path,
                w=W, h=H, bh=tc.DEFAULT_BH, kerr=dc.KERRS[kerr], r_out=r_out, depth=depth, ns_aa=ns_aa, nal=nal,
                hemi=hemi, lensed=lensed, env=lensed, redshift=redshift, light=light, floors=floors)


def banana(build, kerr, depth):
    c = Case(BANANA)
    return dict(build=build, scene=c.scene_path, camera=c.camera_path, w=c.frame_w, h=c.frame_h, bh=FRAME_BH, kerr=kerr,
                r_out=None, depth=depth, ns_aa=16, nal=1, hemi=False, lensed=True, env=True, redshift=True, light=False,
                floors={6: 100, 7: 100})


# name: the case; floors {event: pixels in which it happened at least once, at least}.  Events (rrt_oracle.h
# ro_render_events): [0] camera rays ending on the disk, [1] listed-light shadow rays occluded at a disk
# crossing, [2] hemisphere samples ending on the disk, [3] / [4] bounce rays ending on the disk from a
# delta / a non-delta level, [5] disk-light samples that contributed, [6] environment shadow rays that
# escaped and contributed, [7] escaped camera rays.
# The pixels each case shows, by the restatement (of 6912; the banana frames of 3072):
#   1  [0] 1258  [1] 4261                          2  [0] 694  [2] 4556
#   3  [0] 1254  [1] 5050  [3] 624  [4] 4262       4  [0] 1137  [2] 5117  [3] 445  [4] 4758
#   5  [0] 1243  [1] 4728  [3] 96   [4] 3190  [6] 3838  [7] 527
#   6  [0] 2002  [1] 4082 (the disk-less twin differs in 4057 pixels)
#   7  [0] 1253  [1] 4341  [5] 5103                8  [0] 680  [1] 5255  [3] 334  [4] 4276  [5] 5731
#   9  [6] 805  [7] 2463    10  [6] 808  [7] 2474    11  [6] 766  [7] 1793    12  [6] 792  [7] 1799
# and the adaptive loop stops pixels at 4, 8, 12 and 16 samples (4 and 8 at ns_aa 8; case 6 takes its 4).
CASES = {
    "1_disk_shadow_rays": room(7, "CBspheres_lambertian", "a0.9", 16.0, 1, 16, 4, {0: 300, 1: 300}),
    "2_disk_hemisphere": room(7, "CBspheres_lambertian", "a0", 16.0, 1, 16, 4, {2: 300}, hemi=True),
    "3_disk_bounces_delta": room(7, "CBspheres", "a0.9", 16.0, 4, 16, 2, {3: 32, 4: 100}),
    "4_wide_disk_hemisphere_bounces": room(7, "CBspheres", "a0", 30.0, 3, 8, 2, {2: 300, 3: 32}, hemi=True),
    "5_disk_lensed_env": room(7, "CBspheres", "a0.9", 16.0, 2, 8, 4, {6: 100, 7: 30}, lensed=True),
    "6_disk_beyond_the_scene": room(7, "CBspheres_lambertian", "a0", 60.0, 1, 4, 4, {1: 300}, redshift=False),
    "7_disk_light": room(9, "CBspheres_lambertian", "a0.9", 16.0, 1, 16, 4, {5: 300}, light=True),
    "8_disk_light_bounces": room(9, "CBspheres", "a0", 16.0, 3, 8, 2, {5: 300, 3: 32}, light=True),
    "9_sky_schwarzschild_depth_1": banana(5, None, 1),
    "10_sky_schwarzschild_depth_3": banana(5, None, 3),
    "11_sky_kerr_depth_1": banana(6, FRAME_KERR, 1),
    "12_sky_kerr_depth_3": banana(6, FRAME_KERR, 3),
}
ORDER = sorted(CASES, key=lambda n: int(n.split("_")[0]))


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def configure(r, c, disk=True):
    """The case's scene, camera, map, hole and disk on a context (the GPU's, or a host-only one: the
    disk's r_in resolves on the host).  disk=False: the case's disk-less twin.  Returns the resolved
    r_in in M (None without a disk)."""
    r.set_scene(rrt.SceneFile(c["scene"]))
    r.set_camera(rrt.load_camera(c["camera"]))
    r.set_envmap(Case("env_bunny_96x72_s16").envmap if c["env"] else None)
    bh = c["bh"]
    if c["kerr"] is None:
        r.set_black_hole(bh[:3], bh[3], bh[4], lensed_sky=c["lensed"])
    else:
        r.set_black_hole(bh[:3], bh[3], bh[4], spin=c["kerr"][0], axis=c["kerr"][1], lensed_sky=c["lensed"])
    if c["r_out"] is None or not disk:
        r.set_disk(None)
        return None
    r.set_disk(0.0, c["r_out"], emission=EM, redshift=c["redshift"], light=c["light"])
    return r.get_disk()["r_in"]


def gpu_params(c):
    return rrt.render_params(c["w"], c["h"], ns_aa=c["ns_aa"], max_ray_depth=c["depth"], ns_area_light=c["nal"],
                             samples_per_batch=4, direct_hemisphere=c["hemi"])


def restatement(name, r_in, disk=True):
    """(rgb, count, draws, events) of the case by the restatement at 16 threads, computed once."""
    key = (name, disk)
    if key not in _frames:
        c = CASES[name]
        s = ol.Scene(c["scene"])
        if c["env"]:
            s.set_envmap(Case("env_bunny_96x72_s16").envmap)
        dk = None
        if c["r_out"] is not None and disk:
            dk = dict(r_in=r_in, r_out=c["r_out"], emission=EM, redshift=c["redshift"], light=c["light"])
        p = ol.make_params(c["w"], c["h"], ns_aa=c["ns_aa"], max_ray_depth=c["depth"], ns_area_light=c["nal"],
                           samples_per_batch=4, direct_hemisphere=c["hemi"], bh=c["bh"], kerr=c["kerr"],
                           lensed_sky=c["lensed"], disk=dk)
        _frames[key] = ol.render_events(s, ol.load_camera(c["camera"]), p, 0, 0, c["w"], c["h"], threads=THREADS)
    return _frames[key]


def event_pixels(ev):
    """Per event, the number of pixels in which it happened at least once."""
    return (ev.reshape(-1, ol.N_EVENTS) > 0).sum(0)


def assert_same_frame(got, ref, what):
    rgb, cnt, draws = got
    bad = np.argwhere((u32(rgb) != u32(ref[0])).any(-1) | (cnt != ref[1]) | (draws != ref[2]))
    if len(bad):
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, the first (x, y) = ({x}, {y}): rgb {rgb[y, x]} / "
                             f"{ref[0][y, x]}, count {cnt[y, x]} / {ref[1][y, x]}, draws {draws[y, x]} / {ref[2][y, x]}")


@pytest.mark.parametrize("name", ORDER)
def test_frame_is_the_restatements(gpu, name):
    """One render with RRT_RENDER_DRAWS against the restatement's frame: rgb as uint32, count and draws
    equal on every pixel; the kernel is the expected build; the frame holds what the case is for (the
    floors, on the restatement's event counts); the adaptive loop stops pixels at different counts.
    Pixels per event each case shows, [0]..[7] (the table above CASES names the events):
      1 [1258, 4261, 0, 0, 0, 0, 0, 0]          2 [694, 0, 4556, 0, 0, 0, 0, 0]
      3 [1254, 5050, 0, 624, 4262, 0, 0, 0]     4 [1137, 0, 5117, 445, 4758, 0, 0, 0]
      5 [1243, 4728, 0, 96, 3190, 0, 3838, 527] 6 [2002, 4082, 0, 0, 0, 0, 0, 0]
      7 [1253, 4341, 0, 0, 0, 5103, 0, 0]       8 [680, 5255, 0, 334, 4276, 5731, 0, 0]
      9 [.., 805, 2463]   10 [.., 808, 2474]   11 [.., 766, 1793]   12 [.., 792, 1799]"""
    c = CASES[name]
    r_in = configure(gpu, c)
    rgb, cnt, draws, _ = gpu.render(gpu_params(c), 0, 0, c["w"], c["h"], draws=True)
    kernel = gpu.stats().kernel.decode()
    ref = restatement(name, r_in)
    n = event_pixels(ref[3])
    print(f"{name}: kernel {kernel}; pixels per event {n.tolist()}; counts {np.unique(ref[1]).tolist()}; "
          f"mean {float(ref[0].mean()):.4f}")
    assert ("<true, false, %d," % c["build"]) in kernel, kernel
    for e, floor in c["floors"].items():
        assert n[e] >= floor, (name, e, int(n[e]), floor)
    assert float(ref[0].max()) > 0 and (len(np.unique(ref[1])) >= 2 or c["ns_aa"] <= 4)
    assert_same_frame((rgb, cnt, draws), ref, name)
    if name.startswith("6_"):
        # the disk reaches beyond the room and grows the escape radius; it plays its part: the
        # disk-less twin differs
        configure(gpu, c, disk=False)
        twin = gpu.render(gpu_params(c), 0, 0, c["w"], c["h"], draws=True)[:3]
        assert "<true, false, 7," not in gpu.stats().kernel.decode()
        assert_same_frame(twin, restatement(name, None, disk=False), name + " (disk-less twin)")
        differ = (u32(twin[0]) != u32(rgb)).any(-1) | (twin[1] != cnt) | (twin[2] != draws)
        print(f"  the disk-less twin differs in {int(differ.sum())} pixels")
        assert differ.sum() >= 300


# the disk builds the restatement does not cover (the blackbody colours) next to the two it does
COLOUR_BUILDS = {7: {}, 8: dict(temperature=6000.0), 9: dict(light=True), 10: dict(temperature=6000.0, light=True),
                 11: dict(temperature=6000.0, profile="page-thorne"),
                 12: dict(temperature=6000.0, profile="page-thorne", light=True)}


@pytest.mark.parametrize("build", sorted(COLOUR_BUILDS))
def test_sample_counts_agree_with_the_draws_in_every_disk_build(gpu, build):
    """The adaptive loop's count in every disk build, the blackbody ones included.  Case 7's frame
    (depth 1, ns_aa 16, samples_per_batch 4).  A pixel whose 16 camera rays all end without direct light
    -- on the disk, in the hole or in the black sky: by the restatement's draws, 2 per sample -- takes 2
    draws per sample whatever the disk's colour, so there draws == 2 count in every build, and a pixel
    that stayed black stopped at its first batch.  (V_KERR_DISK_LIGHT reported the wave's largest count
    for every lane and divided rgb by it.)"""
    c = CASES["7_disk_light"]
    r = room(7, "CBspheres_lambertian", "a0.9", 16.0, 1, 16, 4, {})
    r_in = configure(gpu, r)
    key = ("jitter only", r_in)
    if key not in _frames:
        p = ol.make_params(W, H, ns_aa=16, max_ray_depth=1, ns_area_light=4, bh=r["bh"], kerr=r["kerr"],
                           disk=dict(r_in=r_in, r_out=16.0, emission=EM))  # samples_per_batch 32: all 16 samples
        _frames[key] = ol.render(ol.Scene(r["scene"]), ol.load_camera(r["camera"]), p, 0, 0, W, H, threads=THREADS)
    plain = _frames[key]
    jitter_only = (plain[1] == 16) & (plain[2] == 32)
    assert jitter_only.sum() >= 1000, int(jitter_only.sum())
    gpu.set_disk(0.0, 16.0, emission=EM, **COLOUR_BUILDS[build])
    rgb, cnt, draws, _ = gpu.render(gpu_params(c), 0, 0, W, H, draws=True)
    kernel = gpu.stats().kernel.decode()
    assert ("<true, false, %d," % build) in kernel, kernel
    black = jitter_only & ~rgb.any(-1)
    print(f"build {build}: {int(jitter_only.sum())} jitter-only pixels, {int(black.sum())} of them black; counts there "
          f"{np.unique(cnt[jitter_only], return_counts=True)}")
    assert np.array_equal(draws[jitter_only], 2 * cnt[jitter_only].astype(np.uint32))
    assert black.sum() >= 300 and (cnt[black] == 4).all()
    assert len(np.unique(cnt)) >= 3


def test_case_1_through_the_other_entry_points(gpu):
    """Case 1 through rrt_render_tiles_device and a one-member group: the restatement's bits."""
    from test_gpu_disk import group_render, tiles_render
    name = ORDER[0]
    c = CASES[name]
    ref = restatement(name, configure(gpu, c))
    p = gpu_params(c)
    trgb, tcnt = tiles_render(gpu, p)
    assert "<true, false, 7," in gpu.stats().kernel.decode()
    assert np.array_equal(u32(trgb), u32(ref[0])) and np.array_equal(tcnt, ref[1])
    grgb, gcnt = group_render(gpu, p)
    assert np.array_equal(u32(grgb), u32(ref[0])) and np.array_equal(gcnt, ref[1])
