"""GPU: the thin accretion disk (rrt_set_disk, RRT_RAY_DISK, kernel build V_KERR_DISK)
against the CPU rule of tests/disk_check.py, bit for bit: the records of the disk kernels from the
checked disk-less records of the same rays, the frame pixel by pixel from its checked camera records
under either sky rule, every render entry point, the rejected combinations and the command line.
CBspheres with the default hole as Kerr (a/M 0 and 0.9, one tilted axis), the disk ISCO..16 M, and
ISCO..30 M where a chord must hold a crossing and a primitive hit (tests/test_disk_rule.py says why)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import disk_check as dc
import rrt
import trace_check as tc
from golden_cases import GOLD, Case
from test_gpu_lensed_sky import check_kerr_exit
from test_gpu_trace import prims_of

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLI = os.path.join(ROOT, "relativistic-ray-tracer_amd", "rrt_render")
SPHERES = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
BH = tc.DEFAULT_BH
EM = (2.0, 1.0, 0.5)
MISS, HIT, CAPTURED, ESCAPED, DISK = dc.MISS, dc.HIT, dc.CAPTURED, dc.ESCAPED, dc.DISK
W, H = 96, 72
_cache = {}


@pytest.fixture(scope="module")
def gpu():
    r = rrt.Renderer(device=0)
    yield r
    r.close()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def setup(gpu, kerr, r_out=dc.R_OUT, emission=EM, redshift=True, lensed=False, env=False):
    """CBspheres, its camera, the default hole as Kerr; r_out None: no disk.  Returns the Hole."""
    k = dc.KERRS[kerr]
    gpu.set_scene(rrt.SceneFile(SPHERES))
    gpu.set_camera(rrt.load_camera(Case(dc.CAMERA_CASE).camera_path))
    gpu.set_envmap(Case("env_bunny_96x72_s16").envmap if env else None)
    gpu.set_black_hole(BH[:3], BH[3], BH[4], spin=k[0], axis=k[1], lensed_sky=lensed)
    if r_out is None:
        gpu.set_disk(None)
    else:
        gpu.set_disk(0.0, r_out, emission=emission, redshift=redshift)
    return dc.Hole(BH, k)


def disk_of(gpu, hole):
    g = gpu.get_disk()
    return dc.Disk(hole, g["r_in"], g["r_out"], g["emission"], g["redshift"])


def trace(gpu, rset, o, d, **kw):
    if rset == "camera":
        return gpu.trace_camera(W, H, 0, 0, W, H, **kw).ravel()
    return gpu.trace_rays(o, d, **kw)


def diskless(gpu, rset, kerr):
    """(o, d, the checked disk-less closest-hit records) of a ray set under a hole, computed once."""
    key = (rset, kerr)
    if key not in _cache:
        hole = setup(gpu, kerr, r_out=None)
        o, d = dc.gpu_rays(rset, hole, stride=1)
        un = trace(gpu, rset, o, d, mode="lane")
        orc = tc.Oracle(SPHERES, BH, dc.KERRS[kerr])
        tc.check_closest(orc, prims_of("spheres"), o, d, orc.query(o, d), un)
        _cache[key] = (o, d, un)
    return _cache[key]


def differing(a, b):
    return np.flatnonzero([a[i].tobytes() != b[i].tobytes() for i in range(len(a))])


# ------------------------------------------------------------------ records
@pytest.mark.parametrize("r_out", [dc.R_OUT, dc.R_OUT_WIDE])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
@pytest.mark.parametrize("rset", dc.GPU_SETS)
def test_records(gpu, rset, kerr, r_out):
    """Closest-hit records bit for bit from the checked disk-less records; any-hit records their
    status / steps projection; exit mode leaves DISK records alone and treats the others by
    check_kerr_exit; wave per ray stays invalid; removing the disk gives the disk-less records back."""
    o, d, un = diskless(gpu, rset, kerr)
    hole = setup(gpu, kerr, r_out)
    disk = disk_of(gpu, hole)
    assert abs(disk.r_in_m - dc.isco(dc.KERRS[kerr][0])) < 1e-12
    want, kinds = dc.expected_records(hole, disk, o, d, un)
    n = {k: kinds.count(k) for k in ("none", "before", "capture", "prim", "disk_contest", "disk")}
    print(f"{rset}/{kerr}/{r_out} M: {n}")
    got = trace(gpu, rset, o, d, mode="lane")
    bad = differing(got, want)
    assert len(bad) == 0, (bad[:8], got[bad[:2]], want[bad[:2]])
    is_disk = want["status"] == DISK
    assert is_disk.sum() >= 32
    if r_out == dc.R_OUT_WIDE and (rset, kerr) != ("camera", "a0.9"):
        assert n["prim"] + n["disk_contest"] >= 4, n
    assert trace(gpu, rset, o, d).tobytes() == got.tobytes()  # AUTO picks lane per ray
    assert trace(gpu, rset, o, d, any_hit=True, mode="lane").tobytes() == dc.as_any(want).tobytes()
    fl = trace(gpu, rset, o, d, mode="lane", exit=True)
    assert fl[is_disk].tobytes() == want[is_disk].tobytes()
    rest = ~is_disk
    nx = check_kerr_exit(BH, dc.KERRS[kerr], o[rest], d[rest], got[rest], fl[rest])
    print(f"  exit mode, the rays off the disk: miss / hit / captured / escaped = {tuple(nx.values())}")
    assert trace(gpu, rset, o, d, any_hit=True, mode="lane", exit=True).tobytes() == dc.as_any(fl).tobytes()
    with pytest.raises(rrt.RRTError) as e:
        trace(gpu, rset, o, d, mode="wave")
    assert e.value.code == rrt.RRT_E_INVALID
    gpu.set_disk(None)
    assert trace(gpu, rset, o, d, mode="lane").tobytes() == un.tobytes()


@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_no_redshift_gives_unit_normals(gpu, kerr):
    o, d, un = diskless(gpu, "annulus", kerr)
    hole = setup(gpu, kerr, redshift=False)
    disk = disk_of(gpu, hole)
    assert not disk.redshift
    want, _ = dc.expected_records(hole, disk, o, d, un)
    got = gpu.trace_rays(o, d, mode="lane")
    assert len(differing(got, want)) == 0
    nd = got["n"][got["status"] == DISK]
    assert len(nd) >= 32 and np.abs(np.linalg.norm(nd, axis=1) - 1.0).max() < 1e-15
    assert np.abs(np.abs(nd @ np.array(hole.ez)) - 1.0).max() < 1e-15
    # with the redshift |n| = g spreads over the Doppler range
    setup(gpu, kerr)
    gn = np.linalg.norm(gpu.trace_rays(o, d, mode="lane")["n"][got["status"] == DISK], axis=1)
    assert gn.min() < 0.7 and gn.max() > (1.0 if kerr == "a0.9" else 0.9), (gn.min(), gn.max())


@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_disk_beyond_the_scene(gpu, kerr):
    """r_out = 60 M reaches beyond the room's bounding sphere (34.6 M), so the escape radius grows to
    hold the disk.  Rays dropped along -ez from 0.5 above plane points outside the room return DISK
    near the aimed point: a ray passing the hole at impact parameter b is deflected by less than
    4M / b in all, so over the path L it strays by less than L x 4M / b; twice that is allowed."""
    hole = setup(gpu, kerr, r_out=60.0)
    g = np.random.default_rng(5)
    ex, ey, ez, c = (np.array(v) for v in (hole.ex, hole.ey, hole.ez, hole.c))
    rho = hole.m * (36.0 + 22.0 * g.random(256))
    ph = 2 * np.pi * g.random(256)
    tgt = c + (rho * np.cos(ph))[:, None] * ex + (rho * np.sin(ph))[:, None] * ey
    L = 0.5
    o = tgt + L * ez
    lo, hi = np.array([-1.0, 0.0, -1.0]), np.array([1.0, 1.5, 1.0])
    # the whole straight path outside the room: both ends beyond the same face
    out = (((o < lo - 0.05) & (tgt < lo - 0.05)) | ((o > hi + 0.05) & (tgt > hi + 0.05))).any(1)
    assert out.sum() >= 64, out.sum()
    o, tgt, rho = o[out], tgt[out], rho[out]
    d = np.repeat(-ez[None], len(o), 0)
    rec = gpu.trace_rays(o, d, mode="lane")
    assert (rec["status"] == DISK).all(), np.unique(rec["status"], return_counts=True)
    err = np.linalg.norm(rec["hit_p"] - tgt, axis=1)
    tol = 2.0 * L * 4.0 * hole.m / rho
    print(f"{kerr}: max |hit_p - aimed| = {err.max():.2e}, smallest tolerance {tol.min():.2e}")
    assert (err < tol).all(), (err.max(), tol.min())
    assert (np.abs(np.linalg.norm(rec["n"], axis=1) - 1.0) < 0.2).all()  # far out g is near 1


# ------------------------------------------------------------------ the frame
def group_render(gpu, p):
    L = rrt.lib()
    L.rrt_group_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.rrt_group_render.argtypes = [C.c_void_p, C.POINTER(rrt.RenderParams)] + [C.c_uint32] * 4 + [C.c_void_p] * 3
    L.rrt_group_destroy.argtypes = [C.c_void_p]
    arr = (C.c_void_p * 1)(gpu.h)
    g = C.c_void_p()
    assert L.rrt_group_create(arr, 1, C.byref(g)) == rrt.RRT_OK
    rgb, cnt = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.int32)
    rc = L.rrt_group_render(g, C.byref(p), 0, 0, W, H, rgb.ctypes.data, cnt.ctypes.data, None)
    L.rrt_group_destroy(g)
    assert rc == rrt.RRT_OK
    return rgb, cnt


def tiles_render(gpu, p):
    import torch
    ts = 32
    tiles = rrt.partition_tiles(W, H, ts, 0, 1)
    prgb = torch.zeros(len(tiles) * ts * ts * 3, dtype=torch.float32, device="cuda")
    pcnt = torch.zeros(len(tiles) * ts * ts, dtype=torch.int32, device="cuda")
    out_rgb = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    out_cnt = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    gpu.render_tiles_device(p, tiles, ts, prgb.data_ptr(), pcnt.data_ptr(), stream=s)
    gpu.unpack_tiles_device(tiles, ts, W, H, prgb.data_ptr(), pcnt.data_ptr(), out_rgb.data_ptr(), out_cnt.data_ptr(), stream=s)
    torch.cuda.synchronize()
    return out_rgb.cpu().numpy().reshape(H, W, 3), out_cnt.cpu().numpy().reshape(H, W)


@pytest.mark.parametrize("lensed", [False, True])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_frame_is_exact(gpu, kerr, lensed):
    """96 x 72, ns_aa = 1, depth 0: every pixel from its checked camera record.  DISK: the radiance
    formula; HIT: the primitive's emission (the disk-less frame's pixel, the same for every pixel of
    that BSDF); any other: the sky rule in force through rrt_env_eval -- the map along the unbent ray,
    or, lensed, along an ESCAPED ray's exit direction and black otherwise.  The same frame through
    rrt_render_tiles_device, a one-member group and RRT_RENDER_DRAWS."""
    o, d, un = diskless(gpu, "camera", kerr)
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    setup(gpu, kerr, r_out=None, env=True)
    rgb0, _, _, _ = gpu.render(p, 0, 0, W, H)
    hole = setup(gpu, kerr, lensed=lensed, env=True)
    disk = disk_of(gpu, hole)
    want, _ = dc.expected_records(hole, disk, o, d, un)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane", exit=lensed).ravel()
    st = rec["status"]
    is_disk = want["status"] == DISK
    assert rec[is_disk].tobytes() == want[is_disk].tobytes() and (st[~is_disk] != DISK).all()
    if lensed:
        check_kerr_exit(BH, dc.KERRS[kerr], o[~is_disk], d[~is_disk], want[~is_disk], rec[~is_disk])
    else:
        assert rec.tobytes() == want.tobytes()
    rgb, cnt, draws, _ = gpu.render(p, 0, 0, W, H, draws=True)
    assert "<true, false, 7," in gpu.stats().kernel.decode()
    assert (cnt == 1).all() and (draws == 0).all()
    px = rgb.reshape(-1, 3)
    exp = np.zeros_like(px)
    for i in np.flatnonzero(is_disk):
        exp[i] = dc.first_on(dc.crossings(hole, disk, o[i], d[i])).rgb
    hit = st == HIT
    exp[hit] = rgb0.reshape(-1, 3)[hit]
    for b in np.unique(rec["bsdf"][hit]):
        assert len(np.unique(u32(exp[hit & (rec["bsdf"] == b)]), axis=0)) == 1  # an emission per BSDF
    if lensed:
        esc = st == ESCAPED
        if esc.any():
            exp[esc] = gpu.env_eval(-rec["w_out"][esc])
    else:
        sky = (st == MISS) | (st == CAPTURED)
        exp[sky] = gpu.env_eval(d[sky])
    n = {s: int((st == s).sum()) for s in (MISS, HIT, CAPTURED, ESCAPED, DISK)}
    print(f"{kerr} lensed={lensed}: miss / hit / captured / escaped / disk = {tuple(n.values())}")
    assert n[DISK] >= 300 and len(px) - n[DISK] >= 300 and (n[HIT] >= 300 or kerr != "a0")
    bad = np.flatnonzero((u32(px) != u32(exp)).any(1))
    assert len(bad) == 0, (bad[:8], px[bad[:4]], exp[bad[:4]], st[bad[:4]])
    assert len(np.unique(u32(px[is_disk]), axis=0)) >= 100  # a profile, not a constant
    trgb, tcnt = tiles_render(gpu, p)
    assert np.array_equal(u32(trgb), u32(rgb)) and np.array_equal(tcnt, cnt)
    grgb, gcnt = group_render(gpu, p)
    assert np.array_equal(u32(grgb), u32(rgb)) and np.array_equal(gcnt, cnt)


@pytest.mark.parametrize("lensed", [False, True])
def test_frame_the_disk_is_not_in_equals_the_diskless_frame(gpu, lensed):
    """Frames whose camera rays never reach the disk -- the bottom 12 rows (wall hits) and the top 2
    (captured by the hole or lost) of the a/M = 0 frame with the small disk ISCO..8 M; no DISK record, depth 0 -- are the
    frames without a disk bit for bit: V_KERR_DISK against V_KERR and V_KERR_SKY."""
    kerr = "a0"
    p = rrt.render_params(W, H, ns_aa=1, max_ray_depth=0)
    for x0, y0, w, h, hits in ((0, 0, W, 12, True), (0, 70, W, 2, False)):
        setup(gpu, kerr, r_out=8.0, lensed=lensed, env=True)
        rec = gpu.trace_camera(W, H, x0, y0, w, h, mode="lane", exit=lensed)
        assert (rec["status"] != DISK).all() and ((rec["status"] == HIT) == hits).sum() >= 100
        a = gpu.render(p, x0, y0, w, h, draws=True)[:3]
        assert "<true, false, 7," in gpu.stats().kernel.decode()
        setup(gpu, kerr, r_out=None, lensed=lensed, env=True)
        b = gpu.render(p, x0, y0, w, h, draws=True)[:3]
        assert "<true, false, 7," not in gpu.stats().kernel.decode()
        assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert hits or lensed or u32(a[0]).any()  # the reference's sky rule fills every pixel without a hit


def test_disk_lights_the_floor_under_hemisphere_sampling(gpu):
    """Depth 1 with direct_hemisphere: the mean of the floor pixels rises when the disk's emission is
    doubled, and at emission 0 it falls to the disk-less value or below (a dark disk still blocks the
    ceiling light).  Inequalities, no tolerance: the draws are the same in every frame."""
    kerr = "a0"
    p = rrt.render_params(W, H, ns_aa=4, max_ray_depth=1, ns_area_light=4, direct_hemisphere=True)
    wide = rrt.load_camera(Case("cfg1_spheres_480x360_s8").camera_path)  # the whole room: 30.7 degrees across
    setup(gpu, kerr)
    gpu.set_camera(wide)
    rec = gpu.trace_camera(W, H, 0, 0, W, H, mode="lane")
    floor = (rec["status"] == HIT) & (np.abs(rec["hit_p"][..., 1]) < 1e-6)
    assert floor.sum() >= 300 and (rec["status"] == DISK).sum() >= 30

    def mean(emission, r_out=dc.R_OUT):
        setup(gpu, kerr, r_out=r_out, emission=emission)
        gpu.set_camera(wide)
        rgb, _, _, _ = gpu.render(p, 0, 0, W, H)
        return float(rgb[floor].astype(np.float64).mean())

    m0, m1, m2, none = mean((0, 0, 0)), mean((20, 20, 20)), mean((40, 40, 40)), mean(None, r_out=None)
    print(f"floor mean: no disk {none:.5f}, emission 0 {m0:.5f}, 20 {m1:.5f}, 40 {m2:.5f}")
    assert m2 > m1 > m0 and m0 <= none


# ------------------------------------------------------------------ rejected combinations
@pytest.mark.parametrize("name,depth,flags", [("wavefront", 3, rrt.RRT_RENDER_WAVEFRONT), ("deep_sample", 3, rrt.RRT_RENDER_DEEP_SAMPLE),
                                              ("counters", 1, rrt.RRT_RENDER_COUNTERS), ("switch", 1, rrt.RRT_RENDER_NO_ADAPTIVE)])
def test_rejected_combinations(gpu, name, depth, flags):
    setup(gpu, "a0")
    p = rrt.render_params(W, H, ns_aa=2, max_ray_depth=depth, flags=flags)
    with pytest.raises(rrt.RRTError) as e:
        gpu.render(p, 0, 0, 8, 8, counters=name == "counters")
    assert e.value.code == rrt.RRT_E_INVALID
    assert "accretion disk" in str(e.value) or name == "switch"  # the switches are Schwarzschild-only already


def test_schwarzschild_kind_is_rejected(gpu):
    setup(gpu, "a0")
    gpu.set_black_hole(BH[:3], BH[3], BH[4])
    p = rrt.render_params(W, H, ns_aa=1)
    for call in (lambda: gpu.render(p, 0, 0, 8, 8), lambda: gpu.trace_camera(W, H, 0, 0, 8, 8),
                 lambda: gpu.trace_rays(np.array([[0.5, 0.5, 0.5]]), np.array([[0.0, 0.0, -1.0]]))):
        with pytest.raises(rrt.RRTError) as e:
            call()
        assert e.value.code == rrt.RRT_E_INVALID and "spin 0" in str(e.value)
    gpu.set_disk(None)
    gpu.render(p, 0, 0, 8, 8)


# ------------------------------------------------------------------ the command line
def test_cli_disk(tmp_path):
    """rrt_render --disk: exits 0 and writes a picture that differs from the disk-less one and is the
    tonemapped frame the library renders with the same disk."""
    from png_util import read_png
    from test_image_io import tonemap
    dae = os.path.join(GOLD, "dae", "CBspheres_lambertian.dae")
    if not os.path.exists(dae):
        dae = os.path.join(GOLD, "dae", "banana.dae")
    w, h = 64, 48
    args = ["-r", str(w), str(h), "-s", "1", "-m", "0", "--kerr", "0.9"]
    disk = ["--disk", "0", "16", "--disk-emission", "2", "1", "0.5"]
    pngs = {}
    for name, extra in (("disk", disk), ("plain", []), ("flat", disk + ["--disk-no-redshift"])):
        out = str(tmp_path / (name + ".png"))
        r = subprocess.run([CLI] + args + extra + ["-f", out, dae], capture_output=True, text=True, timeout=120)
        print(r.stdout[-300:], r.stderr[-300:])
        assert r.returncode == 0
        pngs[name] = read_png(out)
    assert not np.array_equal(pngs["disk"], pngs["plain"]) and not np.array_equal(pngs["disk"], pngs["flat"])
    scene, cam = rrt.load_collada(dae, w, h)
    g = rrt.Renderer(device=0)
    g.set_scene(scene)
    g.set_camera(rrt.camera_desc(cam))
    g.set_black_hole(spin=0.9)
    g.set_disk(0.0, 16.0, emission=(2.0, 1.0, 0.5))
    rgb, _, _, _ = g.render(rrt.render_params(w, h, ns_aa=1, max_ray_depth=0), 0, 0, w, h)
    g.close()
    assert np.array_equal(pngs["disk"], tonemap(rgb)[::-1].copy().view(np.uint8).reshape(h, w, 4))
    # a Schwarzschild hole with a disk is an error, not a silent disk-less picture
    r = subprocess.run([CLI] + args[:-2] + disk + ["-f", str(tmp_path / "bad.png"), dae], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "spin 0" in r.stderr
