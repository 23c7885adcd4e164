"""GPU: the disk importance-sampled as a light (RRT_DISK_LIGHT, rrt_disk_sample, kernel builds
V_KERR_DISK_LIGHT / V_KERR_DISK_BB_LIGHT) against the CPU rule of
tests/disk_light_check.py: the sampler bit for bit, the disk's term of a pixel bit for bit on top of the
flag-clear frame, the draws, everything the flag must leave alone, agreement with hemisphere sampling in
the flat limit, the entry points, the rejected combinations and the command line.  CBspheres through the
wide camera with the default hole as Kerr (tests/disk_check.py KERRS), the disk ISCO..16 M, frames
96 x 72 (tests/test_disk_light_rule.py counts what the pixel set holds)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import blackbody_check as bb
import disk_check as dc
import disk_light_check as lc
import rrt
import trace_check as tc
from golden_cases import GOLD, Case
from test_gpu_disk import BH, CLI, SPHERES, group_render, tiles_render, u32
from test_gpu_trace import prims_of

pytestmark = pytest.mark.gpu
W, H, NS = lc.W, lc.H, lc.NS_AREA_LIGHT
EM = (2.0, 1.0, 0.5)
T = 6000.0
_sets = {}


@pytest.fixture(scope="module")
def gpu():
    why = lc.parity()
    if why:
        pytest.skip("PARITY PRECONDITION NOT MET (the checker's math.sin / math.cos / math.exp must be the functions "
                    "rrt_glibm.h restates): " + why)
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def setup(gpu, kerr, light, r_out=dc.R_OUT, emission=EM, temperature=None, lensed=False, env=False, bh=BH, r_in=0.0):
    """CBspheres through the wide camera, the hole `bh` as Kerr, the disk r_in..r_out (None: no disk).
    Returns (hole, checker disk)."""
    k = dc.KERRS[kerr]
    gpu.set_scene(rrt.SceneFile(SPHERES))
    gpu.set_camera(rrt.load_camera(Case(lc.WIDE_CASE).camera_path))
    gpu.set_envmap(Case("env_bunny_96x72_s16").envmap if env else None)
    gpu.set_black_hole(bh[:3], bh[3], bh[4], spin=k[0], axis=k[1], lensed_sky=lensed)
    hole = dc.Hole(bh, k)
    if r_out is None:
        gpu.set_disk(None)
        return hole, None
    gpu.set_disk(r_in, r_out, emission=emission, temperature=temperature, light=light)
    got = gpu.get_disk()
    assert got.get("light", False) == light
    return hole, bb.of(hole, got)


def render(gpu, p):
    rgb, cnt, draws, _ = gpu.render(p, 0, 0, W, H, draws=True)
    return rgb, cnt, draws, gpu.stats().kernel.decode()


def same_bits(a, b):
    """Bit-identical, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    ua, ub = (a.view(np.uint64), b.view(np.uint64)) if a.dtype == np.float64 else (a.view(np.uint32), b.view(np.uint32))
    return (ua == ub) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("r_out", [dc.R_OUT, dc.R_OUT_WIDE])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_sampler_matches_the_checker(gpu, kerr, r_out):
    """rrt_disk_sample on 4097 (p, uv) pairs (a wave's tail too): the bits of wi and of pdf.  p uniform in
    the room, 256 of them in the disk's plane and one on the sampled point itself (0 / 0); the draws
    quotients k / 2147483647 as the kernels form them, 0 and 1 among them.  The flag does not matter."""
    hole, disk = setup(gpu, kerr, light=False, r_out=r_out)
    light = lc.Light(hole, disk)
    g = np.random.default_rng(17)
    n = 4097
    lo, hi = np.array([-1.0, 0.0, -1.0]), np.array([1.0, 1.5, 1.0])
    p = lo + (hi - lo) * g.random((n, 3))
    ex, ey, c = (np.array(v) for v in (hole.ex, hole.ey, hole.c))
    p[:256] = c + g.uniform(-0.9, 0.9, (256, 1)) * ex + g.uniform(-0.9, 0.9, (256, 1)) * ey
    uv = g.integers(0, 2147483648, (n, 2)) / lc.RAND_MAX
    uv[256:264] = [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.0, 0.5], [1.0, 0.25], [0.5, 0.0], [0.5, 1.0]]
    x, y = lc.point(light, uv[300][0], uv[300][1])
    p[300] = lc.world(hole, x, y, 0.0)
    wi, pdf = gpu.disk_sample(p, uv)
    want_wi, want_pdf = lc.sample_many(light, p, uv)
    bad = np.flatnonzero(~(same_bits(wi, want_wi).all(1) & same_bits(pdf, want_pdf)))
    assert len(bad) == 0, (bad[:8], wi[bad[:2]], want_wi[bad[:2]], pdf[bad[:2]], want_pdf[bad[:2]])
    n_bad = int((pdf == 0).sum())
    print(f"{kerr} {r_out} M: {n_bad} invalid samples, pdf {pdf[pdf > 0].min():.3g}..{pdf.max():.3g}")
    assert pdf[300] == 0 and (kerr != "a0" or (pdf[:256] == 0).all()) and (pdf[301:] > 0).all()
    gpu.set_disk(0.0, r_out, emission=EM, light=True)
    wi2, pdf2 = gpu.disk_sample(p, uv)
    assert same_bits(wi2, wi).all() and same_bits(pdf2, pdf).all()


# ------------------------------------------------------------------ 2. the pixels
def pixel_set(gpu, kerr, env):
    """The checked pixels of the frame under a hole, computed once: every STRIDE-th pixel whose checked
    camera record is a hit of a diffuse surface with an axis-aligned normal; for each its light samples
    (tests/disk_light_check.py pixel_samples) and, for every sample with a shadow ray, the crossing that
    ray's closest-hit march ends on (None: it does not end on the disk) from its checked disk-less record."""
    key = (kerr, env)
    if key in _sets:
        return _sets[key]
    scene = rrt.SceneFile(SPHERES)
    bsdfs = lc.bsdfs_of(scene)
    first_draw = lc.n_listed_draws(scene, NS, env)
    orc = tc.Oracle(SPHERES, BH, dc.KERRS[kerr])
    prims = prims_of("spheres")
    xs, ys = lc.frame_pixels()
    o, d = lc.camera_rays(Case(lc.WIDE_CASE).camera_path, xs, ys)
    hole, _ = setup(gpu, kerr, light=False, r_out=None)
    un = gpu.trace_rays(o, d, mode="lane")
    tc.check_closest(orc, prims, o, d, orc.query(o, d), un)
    hole, disk = setup(gpu, kerr, light=False)
    cam, _ = dc.expected_records(hole, disk, o, d, un)
    assert gpu.trace_camera(W, H, 0, 0, W, H, mode="lane")[ys, xs].tobytes() == cam.tobytes()
    light = lc.Light(hole, disk)
    px = []
    for i in np.flatnonzero(cam["status"] == dc.HIT):
        if not lc.checkable(bsdfs, int(cam["bsdf"][i]), cam["n"][i]):
            continue
        k = lc.ol.lib().ro_pixel_key(0, int(xs[i]), int(ys[i]))
        px.append((int(xs[i]), int(ys[i]), lc.diffuse_f(bsdfs[int(cam["bsdf"][i])][1]),
                   lc.pixel_samples(light, cam["hit_p"][i], cam["n"][i], k, first_draw, NS)))
    rays = [s for _, _, _, ss in px for s in ss if s.shadow]
    so, sd = np.array([s.o for s in rays]), np.array([s.wi for s in rays])
    setup(gpu, kerr, light=False, r_out=None)
    sun = gpu.trace_rays(so, sd, mode="lane")
    tc.check_closest(orc, prims, so, sd, orc.query(so, sd), sun)
    kinds, ends = [], []
    for j, s in enumerate(rays):
        s.crossing, kind, status = lc.shadow_crossing(hole, disk, so[j], sd[j], sun[j])
        kinds.append(kind)
        ends.append(status)
    n = {k: kinds.count(k) for k in ("none", "before", "capture", "prim", "disk_contest", "disk")}
    n_disk, n_stopped = ends.count(dc.DISK), ends.count(dc.HIT) + ends.count(dc.CAPTURED)
    n_samples = NS * len(px)
    print(f"{kerr} env={env}: {len(px)} checked pixels, {n_samples} samples, {n_samples - len(rays)} without a shadow ray; "
          f"shadow rays: {n_disk} end on the disk, {n_stopped} on a primitive or in the hole, {len(rays) - n_disk - n_stopped} "
          f"nowhere; by kind {n}")
    # the counts tests/test_disk_light_rule.py shows the CPU rule to give
    assert len(px) >= 300 and n_disk >= 200 and n_stopped >= 50
    _sets[key] = (px, first_draw)
    return _sets[key]


@pytest.mark.parametrize("kerr,mode,lensed", [(k, m, False) for k in sorted(dc.KERRS) for m in ("plain", "blackbody")] +
                         [("a0.9", "plain", True)])
def test_pixels_are_the_flag_clear_frame_plus_the_disk_term(gpu, kerr, mode, lensed):
    """ns_aa = 1, depth 1, ns_area_light = 4: pixel_on == float32(pixel_off + D) per channel on every
    checked pixel, pixel_off the same frame with the flag clear and D the checker's disk term; the
    lensed case has the environment map's light in pixel_off and its draws before the disk's."""
    px, first_draw = pixel_set(gpu, kerr, lensed)
    temperature = T if mode == "blackbody" else None
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=1, ns_area_light=NS)
    setup(gpu, kerr, light=False, temperature=temperature, lensed=lensed, env=lensed)
    off, cnt_off, draws_off, name_off = render(gpu, p)
    hole, disk = setup(gpu, kerr, light=True, temperature=temperature, lensed=lensed, env=lensed)
    on, cnt_on, draws_on, name_on = render(gpu, p)
    assert isinstance(disk, bb.Disk) == (mode == "blackbody")
    assert ("<true, false, 8," if temperature else "<true, false, 7,") in name_off
    assert ("<true, false, 10," if temperature else "<true, false, 9,") in name_on
    assert (cnt_on == 1).all() and (cnt_off == 1).all()
    bad, lit, terms = [], 0, []
    for x, y, f, samples in px:
        assert draws_off[y, x] == first_draw and draws_on[y, x] == first_draw + 2 * NS
        D = lc.pixel_term(samples, [lc.crossing_rgb(disk, s.crossing) if s.shadow and s.crossing is not None else None
                                    for s in samples], f)
        want = off[y, x] + D
        terms.append(D)
        lit += bool(D.any())
        if not (u32(on[y, x]) == u32(want)).all():
            bad.append((x, y, on[y, x], want, off[y, x], D))
    terms = np.array(terms)
    print(f"{kerr} {mode} lensed={lensed}: {len(px)} pixels, {lit} with a disk term, D up to {terms.max():.4g}, "
          f"mean {terms.mean():.4g}; kernel {name_on}")
    assert not bad, (len(bad), bad[:4])
    assert lit >= 100 and len(np.unique(u32(terms), axis=0)) >= 100


# ------------------------------------------------------------------ 3. the draws
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_draws(gpu, kerr):
    """ns_aa = 1: the flag adds 2 ns_area_light draws to every pixel that takes direct light (draws_off >
    0), none elsewhere (the disk, the sky, the hole's shadow)."""
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=1, ns_area_light=NS)
    setup(gpu, kerr, light=False)
    _, _, d0, _ = render(gpu, p)
    setup(gpu, kerr, light=True)
    _, _, d1, _ = render(gpu, p)
    lit = d0 > 0
    assert lit.sum() >= 300 and (~lit).sum() >= 30
    assert np.array_equal(d1.astype(np.int64) - d0, np.where(lit, 2 * NS, 0))


# ------------------------------------------------------------------ 4. nothing else moves
def test_depth_0_and_hemisphere_frames_are_the_flag_clear_frames(gpu):
    kerr = "a0.9"
    for kw in (dict(max_ray_depth=0), dict(max_ray_depth=1, direct_hemisphere=True)):
        p = rrt.render_params(W, H, ns_aa=2, ns_area_light=NS, **kw)
        setup(gpu, kerr, light=False)
        a = render(gpu, p)
        setup(gpu, kerr, light=True)
        b = render(gpu, p)
        assert "<true, false, 7," in a[3] and "<true, false, 9," in b[3]
        assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert u32(a[0]).any()


def test_the_disk_lights_the_floor_under_importance_sampling(gpu):
    """The gap this closes: with the flag clear the floor is the same for emission 20 and 40, bit for bit;
    with it set the floor's mean rises with the emission, and at emission 0 it is the flag-clear mean.
    ns_aa = 1: the pixel-centre rays the floor mask is made of (a jittered ray of a floor pixel at the
    disk's outline would see the disk itself)."""
    kerr = "a0"
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=1, ns_area_light=NS)
    setup(gpu, kerr, light=False)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane")
    floor = (rec["status"] == dc.HIT) & (np.abs(rec["hit_p"][..., 1]) < 1e-6)
    assert floor.sum() >= 300

    def frame(emission, light):
        setup(gpu, kerr, light=light, emission=emission)
        return render(gpu, p)[0][floor]

    c20, c40 = frame((20, 20, 20), False), frame((40, 40, 40), False)
    assert np.array_equal(u32(c20), u32(c40))
    s0, s20, s40 = (frame((e, e, e), True) for e in (0, 20, 40))
    m = [float(a.astype(np.float64).mean()) for a in (c20, s0, s20, s40)]
    print(f"floor mean: flag clear {m[0]:.5f}; flag set, emission 0 {m[1]:.5f}, 20 {m[2]:.5f}, 40 {m[3]:.5f}")
    assert np.array_equal(u32(s0), u32(c20)) and m[1] == m[0]
    assert m[3] > m[2] > m[1]


# ------------------------------------------------------------------ 5. the flat limit
def test_agrees_with_hemisphere_sampling_in_the_flat_limit(gpu):
    """A hole of r_s = 1e-4 (M = 5e-5) bends nothing at the room's scale; the disk 6000..16000 M is the
    annulus 0.3..0.8 the default hole's 6..16 M is.  There both estimators of the floor's direct light --
    importance sampling with the flag, hemisphere sampling -- are unbiased for the same integral, and the
    keyed RNG makes the pixels independent: over the N floor pixels the mean of the differences d must
    lie within 5 standard errors, std(d) / sqrt(N), of 0.  The test has power only if the disk's own
    mean contribution is many standard errors: more than 10 is required of the set-up.
    Measured (ns_aa = 8, 807 floor pixels): mean d = -0.0907 = -3.82 se, the disk's share 28.6 se.  That
    d is not the disk's: under this hole the listed light gives the floor 0 under importance sampling
    and 0.076 under hemisphere sampling, with the flag clear too (shadow rays are marched to the end of
    the geodesic, so the light's own quad stops them once the hole captures none).  The second
    assertion takes the disk's light alone, where that term cancels: mean d = -0.0143 = -0.63 se."""
    kerr = "a0"
    bh = (BH[0], BH[1], BH[2], 1e-4, BH[4])
    kw = dict(r_in=6000.0, r_out=16000.0, emission=(40.0, 40.0, 40.0), bh=bh)
    ns_aa = 8
    setup(gpu, kerr, light=False, **kw)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane")
    floor = (rec["status"] == dc.HIT) & (np.abs(rec["hit_p"][..., 1]) < 1e-6)
    p_imp = rrt.render_params(W, H, ns_aa=ns_aa, max_ray_depth=1, ns_area_light=NS)
    p_hem = rrt.render_params(W, H, ns_aa=ns_aa, max_ray_depth=1, ns_area_light=NS, direct_hemisphere=True)
    imp_off = render(gpu, p_imp)[0][floor].astype(np.float64).mean(1)
    hem = render(gpu, p_hem)[0][floor].astype(np.float64).mean(1)
    setup(gpu, kerr, light=False, **dict(kw, emission=(0.0, 0.0, 0.0)))
    hem_dark = render(gpu, p_hem)[0][floor].astype(np.float64).mean(1)  # the same draws, a black disk
    setup(gpu, kerr, light=True, **kw)
    imp_on, cnt, _, name = render(gpu, p_imp)
    assert "<true, false, 9," in name and (cnt == ns_aa).all()
    imp_on = imp_on[floor].astype(np.float64).mean(1)
    n = int(floor.sum())
    d = imp_on - hem
    se = d.std(ddof=1) / math.sqrt(n)
    disk_mean = float((imp_on - imp_off).mean())
    print(f"{n} floor pixels: importance + disk light {imp_on.mean():.5f}, hemisphere {hem.mean():.5f}, flag clear "
          f"{imp_off.mean():.5f}; mean d {d.mean():+.5f}, standard error {se:.5f} ({d.mean() / se:+.2f} se); the disk's "
          f"share {disk_mean:.5f} = {disk_mean / se:.1f} se")
    assert n >= 300 and disk_mean > 10.0 * se
    assert abs(d.mean()) < 5.0 * se
    # the same bound on the disk's light alone: what the flag adds against what the emission adds under
    # hemisphere sampling (the listed light's terms, which the flag leaves alone, cancel in both)
    d2 = (imp_on - imp_off) - (hem - hem_dark)
    se2 = d2.std(ddof=1) / math.sqrt(n)
    print(f"the disk's light alone: flag {disk_mean:.5f}, hemisphere {(hem - hem_dark).mean():.5f}; mean d {d2.mean():+.5f}, "
          f"standard error {se2:.5f} ({d2.mean() / se2:+.2f} se); the listed light: importance {imp_off.mean():.5f}, "
          f"hemisphere {hem_dark.mean():.5f}")
    assert disk_mean > 10.0 * se2 and abs(d2.mean()) < 5.0 * se2


# ------------------------------------------------------------------ 6. entry points and errors
@pytest.mark.parametrize("mode", ["plain", "blackbody"])
def test_every_entry_point_gives_the_same_frame(gpu, mode):
    setup(gpu, "a0.9", light=True, temperature=T if mode == "blackbody" else None)
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=1, ns_area_light=NS)
    rgb, cnt, _, name = render(gpu, p)
    assert ("<true, false, 10," if mode == "blackbody" else "<true, false, 9,") in name
    trgb, tcnt = tiles_render(gpu, p)
    assert np.array_equal(u32(trgb), u32(rgb)) and np.array_equal(tcnt, cnt)
    grgb, gcnt = group_render(gpu, p)
    assert np.array_equal(u32(grgb), u32(rgb)) and np.array_equal(gcnt, cnt)
    crop, ccnt, _, _ = gpu.render(p, 37, 5, 8, 5)
    assert np.array_equal(u32(crop), u32(rgb[5:10, 37:45])) and (ccnt == 1).all()
    deep = rrt.render_params(W, H, ns_aa=1, max_ray_depth=3, ns_area_light=2)
    a, acnt, adraws, name = render(gpu, deep)  # depth >= 2 takes the term at every level through one_bounce
    assert ("<true, false, 10," if mode == "blackbody" else "<true, false, 9,") in name and np.isfinite(a).all()
    if mode == "plain":
        # the restatement's frame bit for bit (tests/test_gpu_deep_builds.py case 8 has the mirror and the
        # glass sphere, jitter and the adaptive loop; the blackbody colour differs in the disk's rgb alone)
        ol = lc.ol
        pr = ol.make_params(W, H, ns_aa=1, max_ray_depth=3, ns_area_light=2, bh=BH, kerr=dc.KERRS["a0.9"],
                            disk=dict(r_in=gpu.get_disk()["r_in"], r_out=dc.R_OUT, emission=EM, light=True))
        ref = ol.render(ol.Scene(SPHERES), ol.load_camera(Case(lc.WIDE_CASE).camera_path), pr, 0, 0, W, H, threads=16)
        assert np.array_equal(u32(a), u32(ref[0])) and np.array_equal(acnt, ref[1]) and np.array_equal(adraws, ref[2])


@pytest.mark.parametrize("name,depth,flags", [("wavefront", 3, rrt.RRT_RENDER_WAVEFRONT), ("deep_sample", 3, rrt.RRT_RENDER_DEEP_SAMPLE),
                                              ("counters", 1, rrt.RRT_RENDER_COUNTERS), ("switch", 1, rrt.RRT_RENDER_NO_ADAPTIVE)])
def test_rejected_combinations(gpu, name, depth, flags):
    setup(gpu, "a0", light=True)
    p = rrt.render_params(W, H, ns_aa=2, max_ray_depth=depth, flags=flags)
    with pytest.raises(rrt.RRTError) as e:
        gpu.render(p, 0, 0, 8, 8, counters=name == "counters")
    assert e.value.code == rrt.RRT_E_INVALID
    assert "accretion disk" in str(e.value) or name == "switch"  # the switches are Schwarzschild-only already


def test_errors(gpu):
    setup(gpu, "a0", light=True)
    for flags in (2, 8, 2 | rrt.RRT_DISK_LIGHT, 8 | rrt.RRT_DISK_LIGHT):  # bits 1 and 3 are still unassigned
        d = rrt.DiskDesc()
        d.r_in, d.r_out, d.flags = 7.0, 16.0, flags
        assert rrt.lib().rrt_set_disk(gpu.h, C.byref(d)) == rrt.RRT_E_INVALID
    assert gpu.get_disk()["light"] and gpu.get_disk()["r_out"] == dc.R_OUT  # a rejected descriptor leaves the disk in force
    p1, uv1 = np.array([[0.2, 0.3, 0.1]]), np.array([[0.5, 0.5]])
    wi, pdf = gpu.disk_sample(np.zeros((0, 3)), np.zeros((0, 2)))  # n == 0: RRT_OK without a launch
    assert wi.shape == (0, 3) and pdf.shape == (0,)
    gpu.set_black_hole(BH[:3], BH[3], BH[4])  # a Schwarzschild-kind spacetime
    p = rrt.render_params(W, H, ns_aa=1)
    for call in (lambda: gpu.disk_sample(p1, uv1), lambda: gpu.render(p, 0, 0, 8, 8)):
        with pytest.raises(rrt.RRTError) as e:
            call()
        assert e.value.code == rrt.RRT_E_INVALID and "spin 0" in str(e.value)
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=0.0)
    gpu.set_disk(None)
    with pytest.raises(rrt.RRTError) as e:
        gpu.disk_sample(p1, uv1)
    assert e.value.code == rrt.RRT_E_INVALID
    gpu.render(p, 0, 0, 8, 8)


# ------------------------------------------------------------------ 7. the command line
def test_cli_disk_light(tmp_path):
    """rrt_render --disk-light: the depth-1 picture differs from the one without it and is the tonemapped
    frame the library renders with the flag; without --disk it is an error."""
    from png_util import read_png
    from test_image_io import tonemap
    dae = os.path.join(GOLD, "dae", "CBspheres_lambertian.dae")
    w, h = 96, 72  # the frame of spheres_96x72_s1: the room with the disk in it (at 64 x 48 the file's camera sees no wall)
    args = ["-r", str(w), str(h), "-s", "1", "-l", "2", "-m", "1", "--kerr", "0.9"]
    disk = ["--disk", "0", "16", "--disk-emission", "20", "10", "5"]
    pngs = {}
    for name, extra in (("light", disk + ["--disk-light"]), ("plain", disk)):
        out = str(tmp_path / (name + ".png"))
        r = subprocess.run([CLI] + args + extra + ["-f", out, dae], capture_output=True, text=True, timeout=120)
        print(r.stdout[-300:], r.stderr[-300:])
        assert r.returncode == 0
        pngs[name] = read_png(out)
    assert not np.array_equal(pngs["light"], pngs["plain"])
    scene, cam = rrt.load_collada(dae, w, h)
    g = rrt.Renderer(device=0)
    g.set_scene(scene)
    g.set_camera(rrt.camera_desc(cam))
    g.set_black_hole(spin=0.9)
    g.set_disk(0.0, 16.0, emission=(20.0, 10.0, 5.0), light=True)
    rgb, _, _, _ = g.render(rrt.render_params(w, h, ns_aa=1, max_ray_depth=1, ns_area_light=2), 0, 0, w, h)
    assert "<true, false, 9," in g.stats().kernel.decode()
    g.close()
    assert np.array_equal(pngs["light"], tonemap(rgb)[::-1].copy().view(np.uint8).reshape(h, w, 4))
    r = subprocess.run([CLI] + args + ["--disk-light", "-f", str(tmp_path / "bad.png"), dae], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--disk" in r.stderr
