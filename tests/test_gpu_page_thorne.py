"""GPU: the Page-Thorne temperature profile of the blackbody disk (RRT_DISK_PROFILE_PAGE_THORNE, kernel
builds V_KERR_DISK_PT / V_KERR_DISK_PT_LIGHT) against the CPU rule of
tests/page_thorne_check.py, bit for bit: rrt_disk_eval on radii and redshifts no camera ray reaches, the
frame pixel by pixel from its checked crossings through every render entry point, the profile's
dependence on the spin, the constants re-resolved when the spin changes, the disk-light build, the
rejected combinations and the command line.  Sizes are tests/test_gpu_blackbody.py's: CBspheres with the
default hole as Kerr (tests/disk_check.py KERRS), the disk ISCO..16 M at 6000 K, frames 96 x 72 at
ns_aa = 1."""
import math
import os
import subprocess

import numpy as np
import pytest

import blackbody_check as bb
import disk_check as dc
import disk_light_check as lc
import page_thorne_check as pt
import rrt
from golden_cases import GOLD, Case
from test_gpu_blackbody import EM, G_EDGES, T, crossing, plain_frame, same_bits
from test_gpu_disk import BH, CLI, H, SPHERES, W, diskless, group_render, setup, tiles_render, u32
from test_gpu_disk_light import NS, pixel_set, render

pytestmark = pytest.mark.gpu
DISK = dc.DISK
PROFILE = "page-thorne"


@pytest.fixture(scope="module")
def gpu():
    why = bb.parity()
    if why:
        pytest.skip("PARITY PRECONDITION NOT MET (the checker's math.log / acos / cos / exp must be the functions "
                    "rrt_glibm.h restates): " + why)
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def setup_pt(gpu, kerr, profile=PROFILE, redshift=True, lensed=False, env=False, light=False):
    """tests/test_gpu_disk.py's set-up with the blackbody disk ISCO..16 M at T; returns (hole, checker disk)."""
    hole = setup(gpu, kerr, r_out=None, lensed=lensed, env=env)
    gpu.set_disk(0.0, dc.R_OUT, emission=EM, redshift=redshift, temperature=T, profile=profile, light=light)
    return hole, pt.of(hole, gpu.get_disk())


def hole_only(gpu, kerr):
    k = dc.KERRS[kerr]
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1])
    return dc.Hole(BH, k)


# ------------------------------------------------------------------ 1. rrt_disk_eval
@pytest.mark.parametrize("kerr,n,redshift", [("a0.9", n, sh) for n in (1, 63, 64, 65, 4097) for sh in (True, False)] +
                         [("a0", 65, True), ("a0", 65, False)])
def test_disk_eval_matches_the_checker(gpu, kerr, n, redshift):
    """r log-spaced over r_in..r_out with r_in itself first (black) and the checker's peak radius second (at
    g = 1: `emission` to rtol 1e-6), then the redshifts 0, inf, NaN and -1 (black), the rest uniform in
    (0.05, 3); n = 1 and the wave tails 63 / 64 / 65; with and without redshift."""
    hole = hole_only(gpu, kerr)
    gpu.set_disk(0.0, dc.R_OUT, emission=EM, temperature=T, profile=PROFILE, redshift=redshift)
    got_disk = gpu.get_disk()
    assert got_disk["profile"] == PROFILE
    disk = pt.of(hole, got_disk)
    assert isinstance(disk, pt.Disk) and disk.redshift == redshift
    r = np.geomspace(got_disk["r_in"], got_disk["r_out"], n) if n > 1 else np.array([got_disk["r_in"]])
    g = np.random.default_rng(n).uniform(0.05, 3.0, n)
    g[0] = 1.0
    if n > 6:
        r[1] = disk.x_peak * disk.x_peak  # in M
        g[1] = 1.0
        g[2:6] = G_EDGES
    got = gpu.disk_eval(r, g)
    want = pt.eval_rgb(hole, disk, r, g)
    assert got.shape == (n, 3) and same_bits(got, want), np.flatnonzero((u32(got) != u32(want)).any(1))[:8]
    assert not got[0].any()  # the inner edge is black, bit for bit
    if n > 6:
        print(f"{kerr} n={n} redshift={redshift}: peak at {r[1]:.4f} M = {r[1] / r[0]:.4f} r_in shows {got[1]}")
        assert np.allclose(got[1], np.asarray(EM, np.float32), rtol=1e-6, atol=0.0)  # the peak shows the emission
        assert not got[2:6].any() or not redshift  # g = 0, inf, NaN, -1: black
        assert np.isfinite(got).all() and got[6:].any(1).sum() > (n - 6) // 2


def test_disk_eval_below_the_inner_edge_is_black(gpu):
    """No disk below r_in, where the bare formula is positive again between the photon orbit and an ISCO
    edge; r = 0, negative and NaN radii too."""
    for kerr, r_in in (("a0.9", 0.0), ("a0", 0.0), ("a0", 7.0)):
        hole = hole_only(gpu, kerr)
        gpu.set_disk(r_in, dc.R_OUT, emission=EM, temperature=T, profile=PROFILE)
        got_disk = gpu.get_disk()
        disk = pt.of(hole, got_disk)
        f = np.array([0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999999, 1.0 - 2.0 ** -52, -1.0, math.nan, 1.0, 1.5])
        r = got_disk["r_in"] * f
        got = gpu.disk_eval(r, np.ones(len(r)))
        assert same_bits(got, pt.eval_rgb(hole, disk, r, np.ones(len(r))))
        assert not got[:-1].any() and got[-1].all()


# ------------------------------------------------------------------ 2. the frame
@pytest.mark.parametrize("kerr,lensed", [(k, False) for k in sorted(dc.KERRS)] + [("a0.9", True)])
def test_frame_is_exact(gpu, kerr, lensed):
    """Every DISK pixel is the checker's colour of its checked crossing; every other pixel is the plain
    disk's frame's; the records are the plain disk's byte for byte; the build is 11; the frame differs
    from the zero-torque frame on at least 300 disk pixels.  The same frame through
    rrt_render_tiles_device, a one-member group and RRT_RENDER_DRAWS, and a region equals the crop."""
    o, d, _ = diskless(gpu, "camera", kerr)
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    rgb0, rec0 = plain_frame(gpu, kerr, lensed, p)
    setup_pt(gpu, kerr, "zero-torque", lensed=lensed, env=True)
    zt, _, _, _ = gpu.render(p, 0, 0, W, H)
    assert "<true, false, 8," in gpu.stats().kernel.decode()
    hole, disk = setup_pt(gpu, kerr, lensed=lensed, env=True)
    assert isinstance(disk, pt.Disk)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", exit=lensed).ravel()
    assert rec.tobytes() == rec0.tobytes()
    rgb, cnt, draws, _ = gpu.render(p, 0, 0, W, H, draws=True)
    assert "<true, false, 11," in gpu.stats().kernel.decode()
    assert (cnt == 1).all() and (draws == 0).all()
    px, exp = rgb.reshape(-1, 3), rgb0.reshape(-1, 3).copy()
    on = np.flatnonzero(rec["status"] == DISK)
    gs = np.zeros(len(on))
    for j, i in enumerate(on):
        c = crossing(kerr, hole, disk, o, d, i)
        assert rec[i].tobytes() == dc.disk_record(c).tobytes()  # the crossing is the record's
        exp[i] = pt.crossing_rgb(disk, c)
        gs[j] = c.g
    bad = np.flatnonzero((u32(px) != u32(exp)).any(1))
    assert len(bad) == 0, (bad[:8], px[bad[:4]], exp[bad[:4]])
    n_col = len(np.unique(u32(px[on]), axis=0))
    n_zt = int((u32(px[on]) != u32(zt.reshape(-1, 3)[on])).any(1).sum())
    # the approaching side is the bluer one: against the colour the same gas shows at g = 1 (the inner
    # edge is cold and dark here, so the extreme redshifts themselves need not be lit)
    bluer = redder = 0
    for j, i in enumerate(on):
        if px[i].all() and abs(gs[j] - 1.0) > 0.02:
            rest = pt.rgb(disk, math.sqrt(crossing(kerr, hole, disk, o, d, i).r2), 1.0).astype(np.float64)
            if not rest.all():
                continue
            up = float(px[i][2]) / float(px[i][0]) > rest[2] / rest[0]
            assert up == (gs[j] > 1.0), (i, gs[j], px[i], rest)
            bluer += up
            redder += not up
    print(f"{kerr} lensed={lensed}: {len(on)} disk pixels, {n_col} colours, {n_zt} differ from zero-torque, g {gs.min():.3f}.."
          f"{gs.max():.3f}, {bluer} lit pixels bluer than at rest, {redder} redder")
    assert len(on) >= 300 and n_col >= 100 and n_zt >= 300
    assert bluer >= 30 and redder >= 30
    off = rec["status"] != DISK
    assert np.array_equal(u32(px[off]), u32(zt.reshape(-1, 3)[off]))
    trgb, tcnt = tiles_render(gpu, p)
    assert np.array_equal(u32(trgb), u32(rgb)) and np.array_equal(tcnt, cnt)
    grgb, gcnt = group_render(gpu, p)
    assert np.array_equal(u32(grgb), u32(rgb)) and np.array_equal(gcnt, cnt)
    crop, ccnt, _, _ = gpu.render(p, 37, 29, 8, 5)
    assert np.array_equal(u32(crop), u32(rgb[29:34, 37:45])) and (ccnt == 1).all()


# ------------------------------------------------------------------ 3., 4. the spin
def pairs(r_in, r_out, n=257, seed=5):
    g = np.random.default_rng(seed)
    return np.geomspace(r_in * 1.01, r_out, n), g.uniform(0.3, 1.5, n)


def test_the_profile_depends_on_the_spin(gpu):
    """The same annulus 7..16 M at a/M = 0 and 0.9, the same (r, g) pairs: the Page-Thorne colours differ,
    the power profile's are the same bits (it has no spin in it)."""
    r, g = pairs(7.0, dc.R_OUT)
    out = {}
    for profile in (PROFILE, "power"):
        for kerr in sorted(dc.KERRS):
            hole = hole_only(gpu, kerr)
            gpu.set_disk(7.0, dc.R_OUT, emission=EM, temperature=T, profile=profile)
            out[profile, kerr] = gpu.disk_eval(r, g)
            assert same_bits(out[profile, kerr], pt.eval_rgb(hole, pt.of(hole, gpu.get_disk()), r, g))
    assert np.array_equal(u32(out["power", "a0"]), u32(out["power", "a0.9"]))
    n_diff = int((u32(out[PROFILE, "a0"]) != u32(out[PROFILE, "a0.9"])).any(1).sum())
    print(f"{n_diff} of {len(r)} pairs differ between a/M = 0 and 0.9")
    assert n_diff == len(r)


@pytest.mark.parametrize("r_in", [0.0, 7.0])
def test_changing_the_spin_re_resolves_the_constants(gpu, r_in):
    """rrt_set_disk at a/M = 0, then the spin to 0.9: rrt_disk_eval is a fresh context's, bit for bit (the
    constants are filled per launch, as r_in = 0 is resolved)."""
    hole_only(gpu, "a0")
    gpu.set_disk(r_in, dc.R_OUT, emission=EM, temperature=T, profile=PROFILE)
    r0, g = pairs(gpu.get_disk()["r_in"], dc.R_OUT)
    before = gpu.disk_eval(r0, g)
    hole = hole_only(gpu, "a0.9")
    got_disk = gpu.get_disk()
    r, g = pairs(got_disk["r_in"], dc.R_OUT)
    got = gpu.disk_eval(r, g)
    fresh = rrt.Renderer(device=0)
    try:
        k = dc.KERRS["a0.9"]
        fresh.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1])
        fresh.set_disk(r_in, dc.R_OUT, emission=EM, temperature=T, profile=PROFILE)
        assert fresh.get_disk() == got_disk
        want = fresh.disk_eval(r, g)
        want0 = fresh.disk_eval(r0, g)
    finally:
        fresh.close()
    assert np.array_equal(u32(got), u32(want)) and got.any(1).all()
    assert same_bits(got, pt.eval_rgb(hole, pt.of(hole, got_disk), r, g))
    assert not np.array_equal(u32(before), u32(want0))  # and the spin did change the answer at the old pairs


# ------------------------------------------------------------------ 5. the light build
def test_light_build_at_depth_0_is_the_frame(gpu):
    kerr = "a0.9"
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    setup_pt(gpu, kerr, env=True)
    a, acnt, _, _ = gpu.render(p, 0, 0, W, H)
    assert "<true, false, 11," in gpu.stats().kernel.decode()
    setup_pt(gpu, kerr, env=True, light=True)
    assert gpu.get_disk()["light"] is True
    b, bcnt, _, _ = gpu.render(p, 0, 0, W, H)
    assert "<true, false, 12," in gpu.stats().kernel.decode()
    assert np.array_equal(u32(a), u32(b)) and np.array_equal(acnt, bcnt) and u32(a).any()


def setup_wide(gpu, kerr, light):
    """tests/test_gpu_disk_light.py's set-up (the wide camera) with the Page-Thorne disk."""
    k = dc.KERRS[kerr]
    gpu.set_scene(rrt.SceneFile(SPHERES))
    gpu.set_camera(rrt.load_camera(Case(lc.WIDE_CASE).camera_path))
    gpu.set_envmap(None)
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1])
    hole = dc.Hole(BH, k)
    gpu.set_disk(0.0, dc.R_OUT, emission=EM, temperature=T, profile=PROFILE, light=light)
    return hole, pt.of(hole, gpu.get_disk())


def test_light_build_under_hemisphere_sampling_is_the_frame(gpu):
    """Under direct_hemisphere the flag changes nothing (§14): build 12's depth-1 frame is build 11's, bit for
    bit, draws included.  Build 12 is the one build that keeps direct_hemisphere out of line;
    build 11 inlines it, as its parent does."""
    kerr = "a0.9"
    p = rrt.render_params(lc.W, lc.H, ns_aa=2, max_ray_depth=1, ns_area_light=NS, direct_hemisphere=True)
    setup_wide(gpu, kerr, False)
    a = render(gpu, p)
    setup_wide(gpu, kerr, True)
    b = render(gpu, p)
    assert "<true, false, 11," in a[3] and "<true, false, 12," in b[3]
    assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert u32(a[0]).any() and (a[2] > 0).sum() >= 300


@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_pixels_are_the_flag_clear_frame_plus_the_disk_term(gpu, kerr, monkeypatch):
    """ns_aa = 1, depth 1, ns_area_light = 4, tests/test_gpu_disk_light.py's pixel set: pixel_on ==
    float32(pixel_off + D) per channel, D the disk-light checker's term with the crossings' colours taken
    from the Page-Thorne checker."""
    monkeypatch.setattr(lc, "crossing_rgb", pt.crossing_rgb)
    px, first_draw = pixel_set(gpu, kerr, False)
    p = rrt.render_params(lc.W, lc.H, ns_aa=1, max_ray_depth=1, ns_area_light=NS)
    setup_wide(gpu, kerr, False)
    off, cnt_off, draws_off, name_off = render(gpu, p)
    hole, disk = setup_wide(gpu, kerr, True)
    on, cnt_on, draws_on, name_on = render(gpu, p)
    assert isinstance(disk, pt.Disk)
    assert "<true, false, 11," in name_off and "<true, false, 12," in name_on
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
    print(f"{kerr}: {len(px)} pixels, {lit} with a disk term, D up to {terms.max():.4g}, mean {terms.mean():.4g}; kernel {name_on}")
    assert not bad, (len(bad), bad[:4])
    assert lit >= 100 and len(np.unique(u32(terms), axis=0)) >= 100


# ------------------------------------------------------------------ 6. rejected combinations
@pytest.mark.parametrize("name,depth,flags", [("wavefront", 3, rrt.RRT_RENDER_WAVEFRONT), ("deep_sample", 3, rrt.RRT_RENDER_DEEP_SAMPLE),
                                              ("counters", 1, rrt.RRT_RENDER_COUNTERS), ("switch", 1, rrt.RRT_RENDER_NO_ADAPTIVE)])
def test_rejected_combinations(gpu, name, depth, flags):
    setup_pt(gpu, "a0")
    p = rrt.render_params(W, H, ns_aa=2, max_ray_depth=depth, flags=flags)
    with pytest.raises(rrt.RRTError) as e:
        gpu.render(p, 0, 0, 8, 8, counters=name == "counters")
    assert e.value.code == rrt.RRT_E_INVALID
    assert "accretion disk" in str(e.value) or name == "switch"  # the switches are Schwarzschild-only already


def test_schwarzschild_kind_is_rejected(gpu):
    setup_pt(gpu, "a0")
    gpu.set_black_hole(BH[:3], BH[3], BH[4])
    p = rrt.render_params(W, H, ns_aa=1)
    for call in (lambda: gpu.render(p, 0, 0, 8, 8), lambda: gpu.trace_camera(W, H, 0, 0, 8, 8),
                 lambda: gpu.disk_eval(np.ones(2), np.ones(2))):
        with pytest.raises(rrt.RRTError) as e:
            call()
        assert e.value.code == rrt.RRT_E_INVALID and "spin 0" in str(e.value)
    gpu.set_disk(None)
    gpu.render(p, 0, 0, 8, 8)


# ------------------------------------------------------------------ 7. the command line
def test_cli_page_thorne_disk(tmp_path):
    """rrt_render --disk 0 16 --disk-temp 6000 --disk-profile page-thorne: exits 0 and writes the tonemapped
    frame the library renders; it differs from the zero-torque picture; an unknown profile name is an error."""
    from png_util import read_png
    from test_image_io import tonemap
    dae = os.path.join(GOLD, "dae", "CBspheres_lambertian.dae")
    w, h = 64, 48
    args = ["-r", str(w), str(h), "-s", "1", "-m", "0", "--kerr", "0.9", "--disk", "0", "16", "--disk-temp", "6000"]
    pngs = {}
    for name in ("page-thorne", "zero-torque"):
        out = str(tmp_path / (name + ".png"))
        r = subprocess.run([CLI] + args + ["--disk-profile", name, "-f", out, dae], capture_output=True, text=True, timeout=120)
        print(r.stdout[-300:], r.stderr[-300:])
        assert r.returncode == 0
        pngs[name] = read_png(out)
    assert not np.array_equal(pngs["page-thorne"], pngs["zero-torque"])
    scene, cam = rrt.load_collada(dae, w, h)
    g = rrt.Renderer(device=0)
    g.set_scene(scene)
    g.set_camera(rrt.camera_desc(cam))
    g.set_black_hole(spin=0.9)
    g.set_disk(0.0, 16.0, temperature=6000.0, profile="page-thorne")
    rgb, _, _, _ = g.render(rrt.render_params(w, h, ns_aa=1, max_ray_depth=0), 0, 0, w, h)
    assert "<true, false, 11," in g.stats().kernel.decode()
    g.close()
    assert np.array_equal(pngs["page-thorne"], tonemap(rgb)[::-1].copy().view(np.uint8).reshape(h, w, 4))
    r = subprocess.run([CLI] + args + ["--disk-profile", "novikov", "-f", str(tmp_path / "bad.png"), dae], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and not os.path.exists(str(tmp_path / "bad.png"))
