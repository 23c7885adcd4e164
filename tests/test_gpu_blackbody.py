"""GPU: the blackbody accretion disk (RRT_DISK_BLACKBODY, rrt_disk_eval, kernel build V_KERR_DISK_BB;
DESIGN.md §13) against the CPU rule of tests/blackbody_check.py, bit for bit: rrt_disk_eval on radii and
redshifts no camera ray reaches, the frame pixel by pixel from its checked crossings through every
render entry point, the flag's absence (the plain disk's frame and records), the rejected combinations
and the command line.  CBspheres with the default hole as Kerr (tests/disk_check.py KERRS), the disk
ISCO..16 M at 6000 K, frames 96 x 72 at ns_aa = 1, depth 0, as tests/test_gpu_disk.py renders them."""
import math
import os
import subprocess

import numpy as np
import pytest

import blackbody_check as bb
import disk_check as dc
import rrt
from golden_cases import GOLD
from test_gpu_disk import BH, CLI, H, W, diskless, group_render, setup, tiles_render, u32

pytestmark = pytest.mark.gpu
EM = (2.0, 1.0, 0.5)
T = 6000.0
DISK = dc.DISK
PROFILES = ("power", "zero-torque")
_cross = {}


@pytest.fixture(scope="module")
def gpu():
    why = bb.parity()
    if why:
        pytest.skip("PARITY PRECONDITION NOT MET (the checker's math.exp must be the exp rrt_glibm.h restates): " + why)
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def setup_bb(gpu, kerr, profile="power", redshift=True, lensed=False, env=False, emission=EM):
    """tests/test_gpu_disk.py's set-up with the blackbody disk ISCO..16 M at T; returns (hole, checker disk)."""
    hole = setup(gpu, kerr, r_out=None, lensed=lensed, env=env)
    gpu.set_disk(0.0, dc.R_OUT, emission=emission, redshift=redshift, temperature=T, profile=profile)
    return hole, bb.of(hole, gpu.get_disk())


def crossing(kerr, hole, disk, o, d, i):
    """The first crossing on the annulus of camera ray i (the same for every colour rule: cached)."""
    key = (kerr, disk.redshift, int(i))
    if key not in _cross:
        _cross[key] = dc.first_on(dc.crossings(hole, disk, o[i], d[i]))
    return _cross[key]


def same_bits(a, b):
    """Bit-identical, a NaN matching any NaN."""
    return ((u32(a) == u32(b)) | (np.isnan(a) & np.isnan(b))).all()


# ------------------------------------------------------------------ rrt_disk_eval
G_EDGES = (0.0, math.inf, math.nan, -1.0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("mode", PROFILES + ("plain", "power-flat"))
def test_disk_eval_matches_the_checker(gpu, mode, n):
    """r log-spaced over r_in..r_out with r_in itself first and 49/36 r_in second (both at g = 1), then the
    redshifts 0, inf, NaN and -1, the rest uniform in (0.05, 3); n = 1 and the wave tails 63 / 64 / 65."""
    kerr = "a0.9"
    k = dc.KERRS[kerr]
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1])
    if mode == "plain":
        gpu.set_disk(0.0, dc.R_OUT, emission=EM)
    else:
        gpu.set_disk(0.0, dc.R_OUT, emission=EM, temperature=T, profile=mode.split("-flat")[0], redshift="flat" not in mode)
    hole = dc.Hole(BH, k)
    got_disk = gpu.get_disk()
    disk = bb.of(hole, got_disk)
    assert isinstance(disk, bb.Disk) == (mode != "plain")
    r = np.geomspace(got_disk["r_in"], got_disk["r_out"], n) if n > 1 else np.array([got_disk["r_in"]])
    g = np.random.default_rng(n).uniform(0.05, 3.0, n)
    g[0] = 1.0
    if n > 6:
        r[1] = got_disk["r_in"] * 49.0 / 36.0
        g[1] = 1.0
        g[2:6] = G_EDGES
    got = gpu.disk_eval(r, g)
    want = bb.eval_rgb(hole, disk, r, g)
    assert got.shape == (n, 3) and same_bits(got, want), np.flatnonzero((u32(got) != u32(want)).any(1))[:8]
    em = np.asarray(EM, np.float32)
    if mode == "plain":  # the refactored plain rule is the old one: emission x (float)(c^3 g^4), as disk_check has it
        c = (got_disk["r_in"] * hole.m) / (r * hole.m)
        with np.errstate(all="ignore"):
            old = em[None] * (((c * c) * c) * ((g * g) * (g * g))).astype(np.float32)[:, None]
        assert same_bits(got, old)
    elif mode == "zero-torque":
        assert not got[0].any()  # the inner edge is black
        assert n < 7 or np.allclose(got[1], em, rtol=1e-6)  # the peak shows the emission
    else:
        assert u32(got[0]).tolist() == u32(em).tolist()  # POWER at r_in, g = 1: the emission bit for bit
    if mode != "plain" and n > 6:
        assert not got[2:6].any() or "flat" in mode  # g = 0, inf, NaN, -1: black
        assert np.isfinite(got).all() and got[6:].any(1).sum() > (n - 6) // 2


def test_disk_eval_of_nothing_launches_nothing(gpu):
    setup_bb(gpu, "a0")
    assert gpu.disk_eval(np.zeros(0), np.zeros(0)).shape == (0, 3)
    gpu.set_disk(None)
    with pytest.raises(rrt.RRTError) as e:
        gpu.disk_eval(np.ones(4), np.ones(4))
    assert e.value.code == rrt.RRT_E_INVALID


# ------------------------------------------------------------------ the frame
def plain_frame(gpu, kerr, lensed, p):
    """(rgb, camera records) of the plain disk's frame."""
    setup(gpu, kerr, lensed=lensed, env=True)
    rgb, _, _, _ = gpu.render(p, 0, 0, W, H)
    assert "<true, false, 7," in gpu.stats().kernel.decode()
    return rgb, gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", exit=lensed).ravel()


@pytest.mark.parametrize("kerr,profile,lensed", [(k, f, False) for k in sorted(dc.KERRS) for f in PROFILES] + [("a0.9", "power", True)])
def test_frame_is_exact(gpu, kerr, profile, lensed):
    """Every DISK pixel is the checker's colour of its checked crossing; every other pixel is the plain
    disk's frame's; the records are the plain disk's byte for byte.  The same frame through
    rrt_render_tiles_device, a one-member group and RRT_RENDER_DRAWS, and a region equals the crop."""
    o, d, _ = diskless(gpu, "camera", kerr)
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    rgb0, rec0 = plain_frame(gpu, kerr, lensed, p)
    hole, disk = setup_bb(gpu, kerr, profile, lensed=lensed, env=True)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", exit=lensed).ravel()
    assert rec.tobytes() == rec0.tobytes()
    rgb, cnt, draws, _ = gpu.render(p, 0, 0, W, H, draws=True)
    assert "<true, false, 8," in gpu.stats().kernel.decode()
    assert (cnt == 1).all() and (draws == 0).all()
    px, exp = rgb.reshape(-1, 3), rgb0.reshape(-1, 3).copy()
    on = np.flatnonzero(rec["status"] == DISK)
    gs = np.zeros(len(on))
    for j, i in enumerate(on):
        c = crossing(kerr, hole, disk, o, d, i)
        assert rec[i].tobytes() == dc.disk_record(c).tobytes()  # the crossing is the record's
        exp[i] = bb.crossing_rgb(disk, c)
        gs[j] = c.g
    bad = np.flatnonzero((u32(px) != u32(exp)).any(1))
    assert len(bad) == 0, (bad[:8], px[bad[:4]], exp[bad[:4]])
    n_col = len(np.unique(u32(px[on]), axis=0))
    hi, lo = px[on[gs.argmax()]].astype(np.float64), px[on[gs.argmin()]].astype(np.float64)
    print(f"{kerr} {profile} lensed={lensed}: {len(on)} disk pixels, {n_col} colours, g {gs.min():.3f}..{gs.max():.3f}, "
          f"B/R {lo[2] / lo[0] if lo[0] else math.nan:.4f} at the smallest g, {hi[2] / hi[0] if hi[0] else math.nan:.4f} at the largest")
    assert len(on) >= 300 and n_col >= 100
    assert hi[2] / hi[0] > lo[2] / lo[0]  # the approaching side is the bluer one
    assert not np.array_equal(u32(px[on]), u32(rgb0.reshape(-1, 3)[on]))
    trgb, tcnt = tiles_render(gpu, p)
    assert np.array_equal(u32(trgb), u32(rgb)) and np.array_equal(tcnt, cnt)
    grgb, gcnt = group_render(gpu, p)
    assert np.array_equal(u32(grgb), u32(rgb)) and np.array_equal(gcnt, cnt)
    crop, ccnt, _, _ = gpu.render(p, 37, 29, 8, 5)
    assert np.array_equal(u32(crop), u32(rgb[29:34, 37:45])) and (ccnt == 1).all()


def test_no_redshift_colours_depend_on_the_radius_alone(gpu):
    kerr = "a0.9"
    o, d, _ = diskless(gpu, "camera", kerr)
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    setup_bb(gpu, kerr, env=True)
    shifted, _, _, _ = gpu.render(p, 0, 0, W, H)
    hole, disk = setup_bb(gpu, kerr, redshift=False, env=True)
    assert not disk.redshift
    rgb, _, _, _ = gpu.render(p, 0, 0, W, H)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane").ravel()
    px = rgb.reshape(-1, 3)
    on = np.flatnonzero(rec["status"] == DISK)
    assert len(on) >= 300
    by_r2 = {}
    for i in on:
        c = crossing(kerr, hole, disk, o, d, i)
        want = bb.rgb(disk, math.sqrt(c.r2), math.nan)  # g is not read
        assert px[i].tobytes() == want.tobytes()
        assert by_r2.setdefault(np.float64(c.r2).tobytes(), px[i].tobytes()) == px[i].tobytes()
    off = rec["status"] != DISK
    assert np.array_equal(u32(px[off]), u32(shifted.reshape(-1, 3)[off]))
    assert (u32(px[on]) != u32(shifted.reshape(-1, 3)[on])).any(1).sum() >= 300


def test_removing_the_flag_returns_the_plain_frame(gpu):
    kerr = "a0"
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    rgb0, rec0 = plain_frame(gpu, kerr, False, p)
    setup_bb(gpu, kerr, env=True)
    rgb1, _, _, _ = gpu.render(p, 0, 0, W, H)
    assert not np.array_equal(u32(rgb1), u32(rgb0))
    rgb2, rec2 = plain_frame(gpu, kerr, False, p)
    assert np.array_equal(u32(rgb2), u32(rgb0)) and rec2.tobytes() == rec0.tobytes()
    assert set(gpu.get_disk()) == {"r_in", "r_out", "emission", "redshift"}


# ------------------------------------------------------------------ rejected combinations
@pytest.mark.parametrize("name,depth,flags", [("wavefront", 3, rrt.RRT_RENDER_WAVEFRONT), ("deep_sample", 3, rrt.RRT_RENDER_DEEP_SAMPLE),
                                              ("counters", 1, rrt.RRT_RENDER_COUNTERS), ("switch", 1, rrt.RRT_RENDER_NO_ADAPTIVE)])
def test_rejected_combinations(gpu, name, depth, flags):
    setup_bb(gpu, "a0")
    p = rrt.render_params(W, H, ns_aa=2, max_ray_depth=depth, flags=flags)
    with pytest.raises(rrt.RRTError) as e:
        gpu.render(p, 0, 0, 8, 8, counters=name == "counters")
    assert e.value.code == rrt.RRT_E_INVALID
    assert "accretion disk" in str(e.value) or name == "switch"  # the switches are Schwarzschild-only already


def test_schwarzschild_kind_is_rejected(gpu):
    setup_bb(gpu, "a0")
    gpu.set_black_hole(BH[:3], BH[3], BH[4])
    p = rrt.render_params(W, H, ns_aa=1)
    for call in (lambda: gpu.render(p, 0, 0, 8, 8), lambda: gpu.trace_camera(W, H, 0, 0, 8, 8),
                 lambda: gpu.disk_eval(np.ones(2), np.ones(2))):
        with pytest.raises(rrt.RRTError) as e:
            call()
        assert e.value.code == rrt.RRT_E_INVALID and "spin 0" in str(e.value)
    gpu.set_disk(None)
    gpu.render(p, 0, 0, 8, 8)


# ------------------------------------------------------------------ the command line
def test_cli_blackbody_disk(tmp_path):
    """rrt_render --disk 0 16 --disk-temp 6000: exits 0 and writes the tonemapped frame the library renders
    with the tint as emission; it differs from the untinted plain disk's; --disk-temp needs --disk."""
    from png_util import read_png
    from test_image_io import tonemap
    dae = os.path.join(GOLD, "dae", "CBspheres_lambertian.dae")
    if not os.path.exists(dae):
        dae = os.path.join(GOLD, "dae", "banana.dae")
    w, h = 64, 48
    args = ["-r", str(w), str(h), "-s", "1", "-m", "0", "--kerr", "0.9"]
    pngs = {}
    for name, extra in (("bb", ["--disk", "0", "16", "--disk-temp", "6000"]), ("plain", ["--disk", "0", "16"]),
                        ("zt", ["--disk", "0", "16", "--disk-temp", "6000", "--disk-profile", "zero-torque"])):
        out = str(tmp_path / (name + ".png"))
        r = subprocess.run([CLI] + args + extra + ["-f", out, dae], capture_output=True, text=True, timeout=120)
        print(r.stdout[-300:], r.stderr[-300:])
        assert r.returncode == 0
        pngs[name] = read_png(out)
    assert not np.array_equal(pngs["bb"], pngs["plain"]) and not np.array_equal(pngs["bb"], pngs["zt"])
    scene, cam = rrt.load_collada(dae, w, h)
    g = rrt.Renderer(device=0)
    g.set_scene(scene)
    g.set_camera(rrt.camera_desc(cam))
    g.set_black_hole(spin=0.9)
    g.set_disk(0.0, 16.0, temperature=6000.0)
    assert g.get_disk()["emission"] == rrt.blackbody_tint(6000.0)
    rgb, _, _, _ = g.render(rrt.render_params(w, h, ns_aa=1, max_ray_depth=0), 0, 0, w, h)
    g.close()
    assert np.array_equal(pngs["bb"], tonemap(rgb)[::-1].copy().view(np.uint8).reshape(h, w, 4))
    for extra in (["--disk-temp", "6000"], ["--disk-profile", "power"]):
        r = subprocess.run([CLI] + args + extra + ["-f", str(tmp_path / "bad.png"), dae], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--disk" in r.stderr
