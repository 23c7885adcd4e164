"""GPU: the moving observer (rrt_set_observer, rrt_observer_eval, kernel build V_KERR_OBS 13 and
rrt_trace_obs_lane_kernel) against the CPU rule of tests/observer_check.py, bit for bit:
rrt_observer_eval on pixel and random directions, the camera records as rrt_trace_rays' for (cam.pos,
d_eff), depth-0 frames pixel by pixel from those records, the identity observer against every older
build, the beaming factors at depth 1 and 3 as one float multiplication, every render entry point, the
launch-time refusals and the command line.

The observer frames: CBspheres_lambertian with the default hole as Kerr (tests/disk_check.py KERRS), the
camera tests/observer_check.py observer_camera -- the wide golden camera's pose with a 50 x 38.5 degree
field of view, 40 M from the hole -- and the velocity 0.4 c0 + 0.1 c1 - 0.2 c2 of the camera's axes.
(The narrow camera of tests/test_gpu_disk.py loses the hole under that velocity: the aberration is 23
degrees, its field of view 6.)  By the CPU rule alone (disk_check.cpu_counts on every third pixel) that
frame holds about 5400 surface hits, 1100 escaping rays and 970 / 420 disk hits (a/M 0.9 / 0, ISCO..16 M)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blackbody_check as bb
import disk_check as dc
import observer_check as oc
import page_thorne_check as pt
import rrt
import trace_check as tc
from golden_cases import GOLD, Case
from test_gpu_deep_builds import CASES, COLOUR_BUILDS, configure, gpu_params
from test_gpu_deep_builds import EM as DEEP_EM
from test_gpu_disk import BH, CLI, EM, H, SPHERES, W, differing, group_render, tiles_render, u32

pytestmark = pytest.mark.gpu
MISS, HIT, CAPTURED, ESCAPED, DISK = dc.MISS, dc.HIT, dc.CAPTURED, dc.ESCAPED, dc.DISK
CAM_M = 40.0
_cross = {}


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def setup(gpu, kerr, r_out=dc.R_OUT, lensed=False, env=True, observer=True, frame="static", beaming=True, **disk):
    """The observer frame's scene, camera, map, hole, disk (r_out None: none) and observer (False: none).
    Returns (hole, camera, the checker's Observer or None)."""
    k = dc.KERRS[kerr]
    hole = dc.Hole(BH, k)
    cam = oc.observer_camera(hole, CAM_M)
    gpu.set_scene(rrt.SceneFile(SPHERES))
    gpu.set_camera(cam)
    gpu.set_envmap(Case("env_bunny_96x72_s16").envmap if env else None)
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1], lensed_sky=lensed)
    if r_out is None:
        gpu.set_disk(None)
    else:
        gpu.set_disk(0.0, r_out, emission=EM, **disk)
    if not observer:
        gpu.set_observer(None)
        return hole, cam, None
    beta = oc.gpu_velocity(list(cam.c2w))
    gpu.set_observer(beta, frame=frame, beaming=beaming)
    return hole, cam, oc.Observer(hole, list(cam.pos), beta, frame)


def camera_rays(cam, ob):
    """(o, n', d_eff, D_v, D) of the frame's pixels by the checker."""
    npr = oc.pixel_directions(cam, W, H)
    d_eff, dv, dd = oc.observer_ray(ob, npr)
    return np.repeat(np.array(list(cam.pos))[None], len(npr), 0), npr, d_eff, dv, dd


def emissions(path):
    """float32 [n_bsdfs, 3]: the emission of every BSDF of a scene file (rrt_bsdf_desc: type, params[14])."""
    sf = rrt.SceneFile(path)
    d = rrt.SceneDesc.from_address(sf.desc())
    out = np.zeros((d.n_bsdfs, 3), np.float32)
    for i in range(d.n_bsdfs):
        if C.c_uint32.from_address(d.bsdfs + 60 * i).value == 1:  # RRT_BSDF_EMISSION
            out[i] = np.ctypeslib.as_array((C.c_float * 3).from_address(d.bsdfs + 60 * i + 4))
    return out


# ------------------------------------------------------------------ 1. rrt_observer_eval
@pytest.mark.parametrize("which", ["case", "6M", "observer"])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_observer_eval_matches_the_checker(gpu, kerr, which):
    """The frame's pixel-centre directions plus 2,048 random ones, both frames, the two cameras of
    tests/test_observer_rule.py and the observer frames' own: d_eff, D_v and D bit for bit; the identity
    passes directions through; nothing launches for n = 0."""
    from test_observer_rule import camera
    k = dc.KERRS[kerr]
    hole = dc.Hole(BH, k)
    cam = oc.observer_camera(hole, CAM_M) if which == "observer" else camera(which, hole)
    gpu.set_camera(cam)
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1])
    beta = oc.gpu_velocity(list(cam.c2w))
    dirs = np.concatenate([oc.pixel_directions(cam, W, H), tc.unit(np.random.default_rng(3).normal(size=(2048, 3)))])
    for frame in (oc.STATIC, oc.COORDINATE):
        gpu.set_observer(beta, frame=frame)
        ob = oc.Observer(hole, list(cam.pos), beta, frame)
        got, want = gpu.observer_eval(dirs), oc.observer_ray(ob, dirs)
        for g, w, name in zip(got, want, ("d_eff", "D_v", "D")):
            bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(dirs), -1).any(1))
            assert len(bad) == 0, (frame, name, len(bad), bad[:4], g[bad[:2]], w[bad[:2]])
    gpu.set_observer((0.0, 0.0, 0.0), frame="coordinate")
    d, dv, dd = gpu.observer_eval(dirs)
    assert np.array_equal(bits(d), bits(dirs)) and (dv == 1.0).all() and (dd == 1.0).all()
    assert gpu.observer_eval(np.zeros((0, 3)))[0].shape == (0, 3)
    gpu.set_observer(None)
    with pytest.raises(rrt.RRTError) as e:
        gpu.observer_eval(dirs[:4])
    assert e.value.code == rrt.RRT_E_INVALID and "observer" in str(e.value)


# ------------------------------------------------------------------ 2. records
@pytest.mark.parametrize("r_out", [None, dc.R_OUT, dc.R_OUT_WIDE])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_records_are_trace_rays_of_d_eff(gpu, kerr, r_out):
    """trace_camera with the observer is byte for byte trace_rays(cam.pos, the checker's d_eff): closest
    hit, any hit and exit mode, with and without a disk; at least 90 % of the records differ from the
    observer-less camera's; trace_rays ignores the observer; wave mode is invalid."""
    hole, cam, ob = setup(gpu, kerr, r_out)
    o, npr, d_eff, _, _ = camera_rays(cam, ob)
    n = {}
    for kw in (dict(), dict(any_hit=True), dict(exit=True), dict(any_hit=True, exit=True)):
        got = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", **kw).ravel()
        want = gpu.trace_rays(o, d_eff, mode="lane", **kw)
        bad = differing(got, want)
        assert len(bad) == 0, (kw, len(bad), bad[:8], got[bad[:2]], want[bad[:2]])
        assert gpu.trace_camera(W, H, 0, 0, W, H, **kw).tobytes() == got.tobytes()  # AUTO picks lane per ray
        n[tuple(kw)] = {s: int((got["status"] == s).sum()) for s in (MISS, HIT, CAPTURED, ESCAPED, DISK)}
        if r_out is not None:
            assert n[tuple(kw)][DISK] >= 32, n
        if kw.get("exit"):
            assert n[tuple(kw)][ESCAPED] >= 32, n
    print(f"{kerr} r_out {r_out}: miss / hit / captured / escaped / disk = {[tuple(v.values()) for v in n.values()]}")
    with pytest.raises(rrt.RRTError) as e:
        gpu.trace_camera(W, H, 0, 0, W, H, mode="wave")
    assert e.value.code == rrt.RRT_E_INVALID
    crop = gpu.trace_camera(W, H, 37, 29, 8, 5, mode="lane")
    assert crop.tobytes() == gpu.trace_camera(W, H, 0, 0, W, H, mode="lane")[29:34, 37:45].tobytes()
    with_obs = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane").ravel()
    rays_with = gpu.trace_rays(o, npr, mode="lane")
    gpu.set_observer(None)
    without = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane").ravel()
    assert len(differing(with_obs, without)) >= 0.9 * W * H
    assert gpu.trace_rays(o, npr, mode="lane").tobytes() == rays_with.tobytes() == without.tobytes()


# ------------------------------------------------------------------ 3. depth-0 frames
def crossing(kerr, r_out, redshift, hole, disk, o, d, i):
    key = (kerr, r_out, redshift, int(i))
    if key not in _cross:
        _cross[key] = dc.first_on(dc.crossings(hole, disk, o[i], d[i]))
    return _cross[key]


DISKS = {"plain": {}, "blackbody": dict(temperature=6000.0, profile="power"),
         "page-thorne": dict(temperature=6000.0, profile="page-thorne")}


@pytest.mark.parametrize("kerr,lensed,rule", [("a0.9", False, "plain"), ("a0.9", True, "plain"), ("a0", True, "blackbody"),
                                              ("a0.9", False, "page-thorne"), ("a0", False, "plain")])
def test_depth_0_frame_is_exact(gpu, kerr, lensed, rule):
    """96 x 72, ns_aa = 1, depth 0: every pixel from its checked record (test_records_are_trace_rays_of_d_eff).
    HIT: the BSDF's emission x (float)w(D_v).  DISK: the colour rule of the disk at (r, g D), r and g those
    of the crossing the record is built from -- by the CPU checkers that tests/test_gpu_blackbody.py and
    tests/test_gpu_page_thorne.py pin against rrt_disk_eval bit for bit (the record's |n| is g only to
    rounding, and rrt_disk_eval takes r in M: neither gives the kernel's operands back exactly).  ESCAPED
    under the lensed rule: rrt_env_eval(exit direction) x (float)w(D), MISS / CAPTURED black; any non-hit
    under the reference's rule: rrt_env_eval(d_eff) x (float)w(D).  Then the same frame without beaming
    (no factor, g as recorded) and with a RRT_DISK_NO_REDSHIFT disk (the bare profile stays bare)."""
    if rule != "plain" and (bb.parity() or pt.parity()):
        pytest.skip("PARITY PRECONDITION NOT MET (the checkers' exp / log must be the ones rrt_glibm.h restates)")
    em = emissions(SPHERES)
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    for beaming, redshift in ((True, True), (False, True), (True, False)):
        hole, cam, ob = setup(gpu, kerr, lensed=lensed, beaming=beaming, redshift=redshift, **DISKS[rule])
        disk = pt.of(hole, gpu.get_disk())
        o, npr, d_eff, dv, dd = camera_rays(cam, ob)
        rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", exit=lensed).ravel()
        assert rec.tobytes() == gpu.trace_rays(o, d_eff, mode="lane", exit=lensed).tobytes()
        rgb, cnt, draws, _ = gpu.render(p, 0, 0, W, H, draws=True)
        assert "<true, false, 13," in gpu.stats().kernel.decode()
        assert (cnt == 1).all() and (draws == 0).all()
        st = rec["status"]
        wv = oc.weight(dv) if beaming else np.ones(len(dv), np.float32)
        wd = oc.weight(dd) if beaming else np.ones(len(dd), np.float32)
        exp = np.zeros((W * H, 3), np.float32)
        hit = st == HIT
        exp[hit] = em[rec["bsdf"][hit]] * wv[hit][:, None]
        on = np.flatnonzero(st == DISK)
        for i in on:
            c = crossing(kerr, dc.R_OUT, redshift, hole, disk, o, d_eff, i)
            assert rec[i].tobytes() == dc.disk_record(c).tobytes()  # the crossing is the record's
            exp[i] = pt.any_rgb(disk, c.r, c.g * dd[i] if beaming else c.g)
        if lensed:
            esc = st == ESCAPED
            exp[esc] = gpu.env_eval(-rec["w_out"][esc]) * wd[esc][:, None]
        else:
            sky = (st == MISS) | (st == CAPTURED)
            exp[sky] = gpu.env_eval(d_eff[sky]) * wd[sky][:, None]
        px = rgb.reshape(-1, 3)
        n = {s: int((st == s).sum()) for s in (MISS, HIT, CAPTURED, ESCAPED, DISK)}
        print(f"{kerr} lensed={lensed} {rule} beaming={beaming} redshift={redshift}: miss / hit / captured / escaped / disk = "
              f"{tuple(n.values())}; lit surface pixels {int((hit & px.any(1)).sum())}")
        bad = np.flatnonzero((u32(px) != u32(exp)).any(1))
        assert len(bad) == 0, (len(bad), bad[:8], px[bad[:4]], exp[bad[:4]], st[bad[:4]])
        assert n[DISK] >= 100 and n[HIT] >= 300 and (n[ESCAPED] if lensed else n[MISS] + n[CAPTURED]) >= 100
        assert len(np.unique(u32(px[on]), axis=0)) >= 50  # a profile, not a constant
        if beaming and redshift:
            full = px.copy()
        elif redshift:  # the factors are really there: the disk and the sky change
            assert (u32(full[on]) != u32(px[on])).any(1).mean() > 0.9
            lit = ~hit & (st != DISK) & px.any(1)
            assert lit.sum() >= 100 and (u32(full[lit]) != u32(px[lit])).any(1).mean() > 0.9


# ------------------------------------------------------------------ 4. the identity observer
def both_ways(gpu, p, w, h, old_build):
    """The frame without an observer and under the identity observer: equal bits, counts and draws; the
    kernels are the old build and build 13."""
    gpu.set_observer(None)
    a = gpu.render(p, 0, 0, w, h, draws=True)[:3]
    old = gpu.stats().kernel.decode()
    gpu.set_observer((0.0, 0.0, 0.0), frame="coordinate")
    b = gpu.render(p, 0, 0, w, h, draws=True)[:3]
    new = gpu.stats().kernel.decode()
    gpu.set_observer(None)
    assert ("<true, false, %d," % old_build) in old or ("kernel<false, %d," % old_build) in old, old
    assert "<true, false, 13," in new, new
    bad = np.argwhere((u32(a[0]) != u32(b[0])).any(-1) | (a[1] != b[1]) | (a[2] != b[2]))
    assert len(bad) == 0, (len(bad), bad[:4], a[0][tuple(bad[0])], b[0][tuple(bad[0])])
    assert a[0].any() and len(np.unique(a[1])) >= 2
    return a


@pytest.mark.parametrize("name", [n for n in CASES if int(n.split("_")[0]) in (1, 3, 4, 5, 7, 8, 11, 12)])
def test_identity_observer_is_the_old_build(gpu, name):
    """Cases 1, 3, 4, 5, 7, 8, 11, 12 of tests/test_gpu_deep_builds.py -- frames the restatement pins: depth
    >= 1, hemisphere light, bounces, the disk light, the lensed sky and the adaptive loop -- under the
    identity observer: build 13 gives the old build's rgb (as uint32), counts and draws."""
    c = CASES[name]
    configure(gpu, c)
    both_ways(gpu, gpu_params(c), c["w"], c["h"], c["build"])


@pytest.mark.parametrize("build", sorted(COLOUR_BUILDS))
def test_identity_observer_is_every_colour_build(gpu, build):
    """The six disk builds on case 7's frame: the run-time colour rule is each build's own (GPU against
    GPU: no checker is involved)."""
    c = CASES["7_disk_light"]
    configure(gpu, c)
    gpu.set_disk(0.0, 16.0, emission=DEEP_EM, **COLOUR_BUILDS[build])
    both_ways(gpu, gpu_params(c), W, H, build)


@pytest.mark.parametrize("depth", [1, 3])
def test_identity_observer_is_plain_kerr(gpu, depth):
    """A Kerr frame without disk or lensed sky (build 3, which runs the shadow rays' occlusion proof)."""
    setup(gpu, "a0.9", r_out=None, env=False, observer=False)
    gpu.set_camera(rrt.load_camera(Case("cfg1_spheres_480x360_s8").camera_path))
    p = rrt.render_params(W, H, ns_aa=8, max_ray_depth=depth, ns_area_light=2, samples_per_batch=4)
    both_ways(gpu, p, W, H, 3)


# ------------------------------------------------------------------ 5. beaming at depth >= 1
@pytest.mark.parametrize("depth,lensed", [(1, False), (3, True)])
def test_beaming_is_one_multiplication(gpu, depth, lensed):
    """ns_aa = 1 at depth 1 and 3: on every pixel whose camera ray does not end on the disk,
    rgb(beaming) == rgb(no beaming) * (float)w bit for bit, w = w(D_v) for surface hits and w(D) for the
    sky, from rrt_observer_eval; the draws are equal on all pixels."""
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=depth, ns_area_light=2)
    hole, cam, ob = setup(gpu, "a0.9", lensed=lensed, beaming=False)
    flat, cnt0, draws0, _ = gpu.render(p, 0, 0, W, H, draws=True)
    setup(gpu, "a0.9", lensed=lensed)
    rgb, cnt, draws, _ = gpu.render(p, 0, 0, W, H, draws=True)
    assert "<true, false, 13," in gpu.stats().kernel.decode()
    assert np.array_equal(draws, draws0) and np.array_equal(cnt, cnt0) and (cnt == 1).all()
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", exit=lensed).ravel()
    _, dv, dd = gpu.observer_eval(oc.pixel_directions(cam, W, H))
    st = rec["status"]
    hit = st == HIT
    w = np.where(hit, oc.weight(dv), oc.weight(dd))
    px, fl = rgb.reshape(-1, 3), flat.reshape(-1, 3)
    off = st != DISK
    bad = np.flatnonzero(off & (u32(px) != u32(fl * w[:, None])).any(1))
    assert len(bad) == 0, (len(bad), bad[:8], px[bad[:4]], fl[bad[:4]], w[bad[:4]], st[bad[:4]])
    lit = hit & fl.any(1)
    print(f"depth {depth} lensed={lensed}: {int(lit.sum())} lit surface pixels, {int((~hit & off & fl.any(1)).sum())} lit sky "
          f"pixels, {int((~off).sum())} disk pixels; w {w.min():.3f} .. {w.max():.3f}")
    assert lit.sum() >= 300 and (draws[hit.reshape(H, W)] > 0).all()
    assert (u32(px[lit]) != u32(fl[lit])).any(1).mean() > 0.9  # the factor is not 1


# ------------------------------------------------------------------ 6. every render entry point
def test_entry_points_agree(gpu):
    """16 spp, samples_per_batch 4, depth 1 under the observer: rrt_render, rrt_render_tiles_device and a
    one-member group agree bit for bit, and the adaptive loop stops pixels at three counts or more."""
    setup(gpu, "a0.9", lensed=True)
    p = rrt.render_params(W, H, ns_aa=16, max_ray_depth=1, ns_area_light=2, samples_per_batch=4)
    rgb, cnt, _, _ = gpu.render(p, 0, 0, W, H)
    assert "<true, false, 13," in gpu.stats().kernel.decode()
    assert len(np.unique(cnt)) >= 3, np.unique(cnt)
    trgb, tcnt = tiles_render(gpu, p)
    assert "<true, false, 13," in gpu.stats().kernel.decode()
    assert np.array_equal(u32(trgb), u32(rgb)) and np.array_equal(tcnt, cnt)
    grgb, gcnt = group_render(gpu, p)
    assert np.array_equal(u32(grgb), u32(rgb)) and np.array_equal(gcnt, cnt)


# ------------------------------------------------------------------ 7. launch-time refusals
@pytest.mark.parametrize("name,depth,flags", [("wavefront", 3, rrt.RRT_RENDER_WAVEFRONT), ("deep_sample", 3, rrt.RRT_RENDER_DEEP_SAMPLE),
                                              ("counters", 1, rrt.RRT_RENDER_COUNTERS), ("switch", 1, rrt.RRT_RENDER_NO_ADAPTIVE),
                                              ("thin_lens", 1, rrt.RRT_RENDER_THIN_LENS)])
def test_forbidden_render_flags(gpu, name, depth, flags):
    setup(gpu, "a0", r_out=None)
    p = rrt.render_params(W, H, ns_aa=2, max_ray_depth=depth, flags=flags)
    with pytest.raises(rrt.RRTError) as e:
        gpu.render(p, 0, 0, 8, 8, counters=name == "counters")
    assert e.value.code == rrt.RRT_E_INVALID and "observer" in str(e.value), str(e.value)


def test_refusals_and_removal(gpu):
    """A Schwarzschild-kind spacetime, a camera inside the static limit and group members with different
    observers are RRT_E_INVALID with a message naming the observer; removing the observer restores the
    observer-less frame bit for bit."""
    p = rrt.render_params(W, H, ns_aa=4, max_ray_depth=1, samples_per_batch=2)
    hole, cam, _ = setup(gpu, "a0", observer=False)
    plain = gpu.render(p, 0, 0, W, H, draws=True)[:3]
    assert "<true, false, 7," in gpu.stats().kernel.decode()
    setup(gpu, "a0")
    moved = gpu.render(p, 0, 0, W, H, draws=True)[:3]
    assert (u32(moved[0]) != u32(plain[0])).any(-1).mean() > 0.5

    def refused(call):
        with pytest.raises(rrt.RRTError) as e:
            call()
        assert e.value.code == rrt.RRT_E_INVALID and "observer" in str(e.value), str(e.value)

    gpu.set_black_hole(BH[:3], BH[3], BH[4])  # Schwarzschild kind
    gpu.set_disk(None)
    for call in (lambda: gpu.render(p, 0, 0, 8, 8), lambda: gpu.trace_camera(W, H, 0, 0, 8, 8),
                 lambda: gpu.observer_eval(np.array([[0.0, 0.0, -1.0]]))):
        refused(call)
    gpu.trace_rays(np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, -1.0]]))  # caller rays: no observer
    setup(gpu, "a0")
    inside = oc.observer_camera(hole, 1.9)  # r = 1.9 M < 2 M: f > 1
    gpu.set_camera(inside)
    for call in (lambda: gpu.render(p, 0, 0, 8, 8), lambda: gpu.trace_camera(W, H, 0, 0, 8, 8)):
        refused(call)
    # two members, two observers
    setup(gpu, "a0")
    other = rrt.Renderer(device=0)
    try:
        setup(other, "a0")
        other.set_observer((0.1, 0.0, 0.0))
        L = rrt.lib()
        L.rrt_group_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.rrt_group_render.argtypes = [C.c_void_p, C.POINTER(rrt.RenderParams)] + [C.c_uint32] * 4 + [C.c_void_p] * 3
        L.rrt_group_destroy.argtypes = [C.c_void_p]
        g = C.c_void_p()
        assert L.rrt_group_create((C.c_void_p * 2)(gpu.h, other.h), 2, C.byref(g)) == rrt.RRT_OK
        rgb, cnt = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.int32)
        rc = L.rrt_group_render(g, C.byref(p), 0, 0, W, H, rgb.ctypes.data, cnt.ctypes.data, None)
        msg = L.rrt_last_error(gpu.h).decode()
        L.rrt_group_destroy(g)
        assert rc == rrt.RRT_E_INVALID and "observer" in msg, (rc, msg)
    finally:
        other.close()
    setup(gpu, "a0")
    gpu.set_observer(None)
    again = gpu.render(p, 0, 0, W, H, draws=True)[:3]
    assert "<true, false, 7," in gpu.stats().kernel.decode()
    assert np.array_equal(u32(again[0]), u32(plain[0])) and np.array_equal(again[1], plain[1]) and np.array_equal(again[2], plain[2])


# ------------------------------------------------------------------ 8. the command line
def test_cli_observer(tmp_path):
    """rrt_render --kerr --disk --lensed-sky --observer-velocity writes the PNG of the API frame's tonemap;
    --observer-no-beaming and --observer-frame change the picture; without --kerr it fails with its message."""
    from png_util import read_png
    from test_image_io import tonemap
    dae = os.path.join(GOLD, "dae", "CBspheres_lambertian.dae")
    if not os.path.exists(dae):
        dae = os.path.join(GOLD, "dae", "banana.dae")
    w, h = 64, 48
    vel = (0.02, 0.01, -0.15)  # mostly forward: the room stays in view (no map: the sky is black)
    args = ["-r", str(w), str(h), "-s", "1", "-m", "0", "--kerr", "0.9", "--disk", "0", "16", "--disk-emission", "2", "1", "0.5",
            "--lensed-sky"]
    obs = ["--observer-velocity"] + [str(v) for v in vel]
    pngs = {}
    for name, extra in (("obs", obs), ("plain", []), ("flat", obs + ["--observer-no-beaming"]),
                        ("coord", obs + ["--observer-frame", "coordinate"])):
        out = str(tmp_path / (name + ".png"))
        r = subprocess.run([CLI] + args + extra + ["-f", out, dae], capture_output=True, text=True, timeout=120)
        print(r.stdout[-300:], r.stderr[-300:])
        assert r.returncode == 0
        pngs[name] = read_png(out)
    assert not np.array_equal(pngs["obs"], pngs["plain"]) and not np.array_equal(pngs["obs"], pngs["flat"])
    scene, cam = rrt.load_collada(dae, w, h)
    g = rrt.Renderer(device=0)
    g.set_scene(scene)
    g.set_camera(rrt.camera_desc(cam))
    g.set_black_hole(spin=0.9, lensed_sky=True)
    g.set_disk(0.0, 16.0, emission=(2.0, 1.0, 0.5))
    p = rrt.render_params(w, h, ns_aa=1, max_ray_depth=0)
    for name, kw in (("obs", {}), ("flat", dict(beaming=False)), ("coord", dict(frame="coordinate"))):
        g.set_observer(vel, **kw)
        rgb, _, _, _ = g.render(p, 0, 0, w, h)
        assert np.array_equal(pngs[name], tonemap(rgb)[::-1].copy().view(np.uint8).reshape(h, w, 4)), name
    g.close()
    no_kerr = [v for i, v in enumerate(args) if i not in (args.index("--kerr"), args.index("--kerr") + 1)]
    r = subprocess.run([CLI] + no_kerr + obs + ["-f", str(tmp_path / "bad.png"), dae], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--observer-velocity needs --kerr" in r.stderr
