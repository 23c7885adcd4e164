"""The restatement's exit mode, accretion disk and disk light (oracle/restate rrt_oracle.c: DESIGN.md
§11, §12, §14) against the independent numpy checkers, on the CPU.

tests/test_gpu_deep_builds.py compares whole GPU frames at depth >= 1 with ro_render bit for bit.  A copy
of the kernel could be wrong the same way as the kernel, so the new C is pinned here against
tests/disk_check.py, tests/exit_check.py and tests/disk_light_check.py, which work from ro_kerr_chain /
their own numpy stepper and share no code with it: the records of the new ray query, the depth-0 frames
pixel by pixel, the disk light's identity at depth 1, and everything the disk must leave alone."""
import math
import os

import numpy as np
import pytest

import disk_check as dc
import disk_light_check as lc
import exit_check as xc
import oracle_lib as ol
import rrt
import trace_check as tc
from golden_cases import GOLD, Case
from test_gpu_lensed_sky import FRAME_BH, FRAME_KERR
from test_gpu_trace import HOLES, KERRS, RAYS, SCENES, SETS

SPHERES_L = os.path.join(GOLD, "scenes", "CBspheres_lambertian.rrts")
BH = tc.DEFAULT_BH
EM = (2.0, 1.0, 0.5)
MISS, HIT, CAPTURED, ESCAPED, DISK = dc.MISS, dc.HIT, dc.CAPTURED, dc.ESCAPED, dc.DISK
THREADS = 16
_cache = {}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def disk_of(kerr, r_out, **kw):
    """make_params' disk dict for a hole of dc.KERRS: ISCO..r_out M."""
    return dict(r_in=dc.isco(dc.KERRS[kerr][0]), r_out=r_out, emission=kw.pop("emission", EM), **kw)


def scene_of(path, env=False):
    key = ("scene", path, env)
    if key not in _cache:
        s = ol.Scene(path)
        if env:
            s.set_envmap(Case("env_bunny_96x72_s16").envmap)
        _cache[key] = s
    return _cache[key]


def hit_records(q):
    """rrt.HIT_DTYPE records (what the checkers read and build) of ro_ray_query's records: w_out and prim
    are not in the restatement's record and stay 0 / -1; an ESCAPED record's w_out is minus its e."""
    out = np.zeros(len(q), rrt.HIT_DTYPE)
    out["prim"] = -1
    for f in ("status", "steps", "bsdf", "t", "hit_p", "n"):
        out[f] = q[f]
    esc = q["status"] == ESCAPED
    out["w_out"][esc] = -q["e"][esc]
    return out


def assert_same_records(got, want, what):
    """Status, steps and bsdf equal; t, hit_p, n (and an ESCAPED record's direction) bit for bit."""
    g = hit_records(got)
    for f in ("status", "steps", "bsdf"):
        bad = np.flatnonzero(g[f] != want[f])
        assert len(bad) == 0, (what, f, bad[:8], g[bad[:2]], want[bad[:2]])
    for f in ("t", "hit_p", "n"):
        bad = np.flatnonzero((tc.bits(g[f]).reshape(len(g), -1) != tc.bits(want[f]).reshape(len(g), -1)).any(1))
        assert len(bad) == 0, (what, f, bad[:8], g[bad[:2]], want[bad[:2]])
    esc = want["status"] == ESCAPED
    assert tc.same(g["w_out"][esc], want["w_out"][esc]), (what, "exit direction")
    assert not tc.bits(got["e"][~esc]).any(), (what, "an exit direction on a record that is not ESCAPED")


# ------------------------------------------------------------------ disk queries
def root_esc2(scene, hole):
    """kerr_set_escape: the farthest root-box corner from the hole, at least 4M, squared."""
    boxes, _, _ = scene.bvh()
    m3 = [max(abs(boxes[0][k] - hole.c[k]), abs(boxes[0][3 + k] - hole.c[k])) for k in range(3)]
    return max((m3[0] * m3[0] + m3[1] * m3[1]) + m3[2] * m3[2], (4.0 * hole.m) * (4.0 * hole.m))


def check_diskless(scene, hole, o, d, un, answers):
    """The new query's disk-less Kerr records against the restatement's older entry points alone
    (dc.cpu_diskless: ro_query's answer located on ro_kerr_chain's rows): status; a hit's row, t (to the
    1e-9 the locating allows), hit_p, n and bsdf bit for bit; a capture's row.  A MISS must end as a march
    can: on its budget (the swept angle, by the chain's own), or at a step that starts beyond the escape
    radius with no earlier row outgoing out there."""
    esc2 = root_esc2(scene, hole)
    for i in range(len(o)):
        st, steps, t, rows, extra = dc.cpu_diskless(None, None, hole, o[i], d[i], answers[i])
        r = un[i]
        where = f"ray {i}: {r}"
        assert (int(r["status"]) == HIT) == (st == HIT) and int(r["status"]) in (MISS, HIT, CAPTURED), where
        if st == HIT:
            hit, hp, nn, bsdf = answers[i]
            assert int(r["steps"]) == steps and abs(float(r["t"]) - t) < 1e-9, (where, steps, t)
            assert tc.same(r["hit_p"], hp) and tc.same(r["n"], nn) and int(r["bsdf"]) == bsdf, where
        elif int(r["status"]) == CAPTURED:
            assert st == CAPTURED and int(r["steps"]) == steps, (where, steps)
        else:
            # (the chain has no budget: it may show a capture on a row the march never takes)
            k = int(r["steps"])
            assert 1 <= k <= hole.max_steps and (st == MISS or k < steps), where
            if xc.kerr_budget_end(hole.bh, hole.kerr, o[i], d[i], k, hole.max_steps):
                assert k == 1 or extra[k - 2, 0] < 2.0 * math.pi, where
                continue
            q0, _ = dc.kerr_init(hole, o[i], d[i])
            q = np.vstack([[q0], rows[:, 8:11]])  # q[j]: the state step j starts from
            assert q[k - 1] @ q[k - 1] > esc2, where
            for j in range(k - 1):
                if q[j] @ q[j] > esc2:
                    step = q[j + 1] - q[j]
                    assert q[j] @ step < 1e-6 * np.linalg.norm(q[j]) * np.linalg.norm(step), (where, j)


def diskless(rset, kerr):
    """(scene, hole, o, d, answers, the checked disk-less records) of a ray set under a hole, once."""
    key = ("diskless", rset, kerr)
    if key not in _cache:
        scene = scene_of(SPHERES_L)
        hole = dc.Hole(BH, dc.KERRS[kerr])
        o, d = dc.gpu_rays(rset, hole)  # the camera at stride 3
        orc = tc.Oracle(SPHERES_L, BH, dc.KERRS[kerr])
        answers = orc.query(o, d)
        un = ol.ray_query(scene, ol.make_params(1, 1, bh=BH, kerr=dc.KERRS[kerr]), o, d)
        check_diskless(scene, hole, o, d, un, answers)
        _cache[key] = (scene, hole, o, d, answers, un)
    return _cache[key]


@pytest.mark.parametrize("r_out", [dc.R_OUT, dc.R_OUT_WIDE])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
@pytest.mark.parametrize("rset", dc.GPU_SETS)
def test_disk_queries(rset, kerr, r_out):
    """ro_ray_query with the disk: closest-hit records equal dc.expected_records built on the checked
    disk-less records -- status, steps, bsdf and the disk's rgb exactly, t, hit_p and n bit for bit; the
    any-hit records are their status / steps projection; the counts per kind are dc.cpu_counts'."""
    scene, hole, o, d, answers, un = diskless(rset, kerr)
    disk = dc.Disk(hole, dc.isco(dc.KERRS[kerr][0]), r_out, EM)
    want, kinds = dc.expected_records(hole, disk, o, d, hit_records(un))
    p = ol.make_params(1, 1, bh=BH, kerr=dc.KERRS[kerr], disk=disk_of(kerr, r_out))
    got = ol.ray_query(scene, p, o, d)
    assert_same_records(got, want, (rset, kerr, r_out))
    is_disk = want["status"] == DISK
    for i in np.flatnonzero(is_disk):
        c = dc.first_on(dc.crossings(hole, disk, o[i], d[i]))
        assert np.array_equal(u32(got["rgb"][i]), u32(c.rgb)), (i, got["rgb"][i], c.rgb)
    assert not u32(got["rgb"][~is_disk]).any()
    n = {k: kinds.count(k) for k in ("none", "before", "capture", "prim", "disk_contest", "disk")}
    cpu = dc.cpu_counts(None, None, hole, disk, o, d, answers)
    print(f"{rset}/{kerr}/{r_out} M: {n}; cpu_counts {cpu}")
    assert int(is_disk.sum()) == cpu["disk"] and n["prim"] + n["disk_contest"] == cpu["contest"], (n, cpu)
    assert cpu["disk"] >= 32
    # any-hit: status and steps alone
    any_ = ol.ray_query(scene, p, o, d, any_hit=True)
    assert np.array_equal(any_["status"], want["status"]) and np.array_equal(any_["steps"], want["steps"])
    for f in ("t", "hit_p", "n", "rgb", "e"):
        assert not any_[f].any(), f
    assert (any_["bsdf"] == -1).all()
    # no redshift: the same records with g = 1 (unit normals, the bare profile)
    flat = dc.Disk(hole, disk.r_in_m, r_out, EM, redshift=False)
    want_f, _ = dc.expected_records(hole, flat, o, d, hit_records(un))
    got_f = ol.ray_query(scene, ol.make_params(1, 1, bh=BH, kerr=dc.KERRS[kerr], disk=disk_of(kerr, r_out, redshift=False)), o, d)
    assert_same_records(got_f, want_f, (rset, kerr, r_out, "no redshift"))
    for i in np.flatnonzero(is_disk)[:64]:
        assert np.array_equal(u32(got_f["rgb"][i]), u32(dc.first_on(dc.crossings(hole, flat, o[i], d[i])).rgb))


def test_disk_under_a_schwarzschild_hole_is_an_error():
    scene = scene_of(SPHERES_L)
    cam = ol.load_camera(Case(dc.CAMERA_CASE).camera_path)
    p = ol.make_params(8, 8, bh=BH, disk=dict(r_in=6.0, r_out=16.0))
    with pytest.raises(RuntimeError):
        ol.render(scene, cam, p, 0, 0, 8, 8, threads=1)
    with pytest.raises(RuntimeError):
        ol.render_events(scene, cam, p, 0, 0, 8, 8, threads=1)
    with pytest.raises(RuntimeError):
        ol.ray_query(scene, p, [[0.5, 0.5, 0.5]], [[0.0, 0.0, -1.0]])
    p = ol.make_params(8, 8, bh=BH, kerr=dc.KERRS["a0"], disk=dict(r_in=16.0, r_out=16.0))
    with pytest.raises(RuntimeError):
        ol.render(scene, cam, p, 0, 0, 8, 8, threads=1)


def test_a_caller_with_the_base_record_is_left_alone():
    """The extension fields are appended to ro_params; a caller built against the base record owns no
    byte of them.  ro_params_default writes nothing beyond the base record and leaves ext 0, and with ext
    0 no entry point reads beyond it: a record followed by 0xA5 bytes (a disk switched on, by its bits)
    renders and queries as the same settings through make_params."""
    import ctypes as C
    size, base = C.sizeof(ol.Params), ol.Params.lensed_sky.offset
    assert base == ol.Params.ext.offset + 4 and size > base
    buf = (C.c_ubyte * size)(*([0xA5] * size))
    p = C.cast(buf, C.POINTER(ol.Params)).contents
    ol.lib().ro_params_default(C.byref(p))
    assert bytes(buf[base:]) == b"\xa5" * (size - base) and p.ext == 0 and p.ns_aa == 1 and p.illum == 2
    k = dc.KERRS["a0.9"]
    p.frame_w, p.frame_h, p.ns_aa, p.bh_kind, p.bh_spin = 32, 24, 2, 1, k[0]
    p.bh_axis[0], p.bh_axis[1], p.bh_axis[2] = k[1]
    assert p.disk_on != 0 and p.lensed_sky != 0  # what a reader beyond the base record would see
    scene = scene_of(SPHERES_L)
    cam = ol.load_camera(Case(dc.CAMERA_CASE).camera_path)
    a = ol.render(scene, cam, p, 0, 0, 32, 24, threads=2)[:3]
    b = ol.render(scene, cam, ol.make_params(32, 24, ns_aa=2, bh=BH, kerr=k), 0, 0, 32, 24, threads=2)[:3]
    assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    o, d = RAYS["interior"]
    assert ol.ray_query(scene, p, o[:64], d[:64]).tobytes() == ol.ray_query(scene, ol.make_params(1, 1, bh=BH, kerr=k), o[:64], d[:64]).tobytes()
    assert bytes(buf[base:]) == b"\xa5" * (size - base)
    q = ol.Params()
    ol.lib().ro_params_default_ext(C.byref(q))
    assert q.ext == 0x524F5831 and not bytes(q)[base:].strip(b"\0")


# ------------------------------------------------------------------ exit queries
@pytest.mark.parametrize("hole", sorted(HOLES))
@pytest.mark.parametrize("scene,rset", SETS)
def test_exit_queries_schwarzschild(scene, rset, hole):
    """The exit-mode records of the Schwarzschild stepper equal xc.expected_exit_records on the numpy
    stepper's chains (escape row j*, exit direction), built on the unflagged records -- themselves the
    restatement's older answers (ro_query: hit, hit_p, n, bsdf)."""
    bh = HOLES[hole]
    o, d = RAYS[rset]
    sc = scene_of(SCENES[scene])
    un = ol.ray_query(sc, ol.make_params(1, 1, bh=bh), o, d)
    answers = tc.Oracle(SCENES[scene], bh).query(o, d)
    for i in range(len(o)):
        hit, hp, nn, bsdf = answers[i]
        assert (int(un[i]["status"]) == HIT) == hit
        if hit:
            assert tc.same(un[i]["hit_p"], hp) and tc.same(un[i]["n"], nn) and int(un[i]["bsdf"]) == bsdf
    want = xc.expected_exit_records(xc.Chains(bh, o, d), hit_records(un))
    p = ol.make_params(1, 1, bh=bh, lensed_sky=True)
    fl = ol.ray_query(sc, p, o, d)
    assert_same_records(fl, want, (scene, rset, hole))
    n = {s: int((want["status"] == s).sum()) for s in (MISS, HIT, CAPTURED, ESCAPED)}
    print(f"{scene}/{rset}/{hole}: miss / hit / captured / escaped = {tuple(n.values())}")
    if scene == "spheres" and hole == "default":
        assert rset != "outward" or n[ESCAPED] >= 128, n
        assert rset != "aimed" or n[CAPTURED] >= 256, n
    any_ = ol.ray_query(sc, p, o, d, any_hit=True)
    assert np.array_equal(any_["status"], want["status"]) and np.array_equal(any_["steps"], want["steps"])
    esc = want["status"] == ESCAPED
    assert tc.same(any_["e"][esc], fl["e"][esc]) and not any_["hit_p"].any() and not any_["t"].any()


@pytest.mark.parametrize("kerr", sorted(KERRS))
@pytest.mark.parametrize("scene,rset", SETS)
def test_exit_queries_kerr(scene, rset, kerr):
    """As check_kerr_exit of tests/test_gpu_lensed_sky.py: HIT / CAPTURED records are the unflagged ones;
    an ESCAPED record's direction is the unit chord of the restated chain's exit row (xc.kerr_exit_row);
    a MISS stays only where the chain shows a budget end (xc.kerr_budget_end)."""
    o, d = RAYS[rset]
    k = KERRS[kerr]
    sc = scene_of(SCENES[scene])
    un = ol.ray_query(sc, ol.make_params(1, 1, bh=BH, kerr=k), o, d)
    p = ol.make_params(1, 1, bh=BH, kerr=k, lensed_sky=True)
    fl = ol.ray_query(sc, p, o, d)
    max_steps = 4 * tc.steps_of(BH[4])
    n = {MISS: 0, HIT: 0, CAPTURED: 0, ESCAPED: 0}
    for i in range(len(o)):
        st, steps = int(fl[i]["status"]), int(fl[i]["steps"])
        where = f"ray {i}: {fl[i]} unflagged {un[i]}"
        n[st] += 1
        if int(un[i]["status"]) in (HIT, CAPTURED):
            assert fl[i].tobytes() == un[i].tobytes(), where
            continue
        assert st in (MISS, ESCAPED) and steps == int(un[i]["steps"]), where
        if st == MISS:
            assert fl[i].tobytes() == un[i].tobytes(), where
            assert xc.kerr_budget_end(BH, k, o[i], d[i], steps, max_steps), where
            continue
        row = xc.kerr_exit_row(BH, k, o[i], d[i], steps, max_steps)
        assert row is not None and tc.same(fl[i]["e"], -row[1]), (where, row)
        assert not fl[i]["hit_p"].any() and not fl[i]["n"].any() and fl[i]["t"] == 0 and fl[i]["bsdf"] == -1, where
    print(f"{scene}/{rset}/kerr {kerr}: miss / hit / captured / escaped = {tuple(n.values())}")
    if rset == "outward":
        assert n[ESCAPED] >= 128, n
    any_ = ol.ray_query(sc, p, o, d, any_hit=True)
    assert np.array_equal(any_["status"], fl["status"]) and np.array_equal(any_["steps"], fl["steps"])
    assert tc.same(any_["e"], fl["e"])


# ------------------------------------------------------------------ the environment lookup
PI = 3.14159265358979323  # CGL misc.h:11


def env_bilerp(tex, xx, yy):
    """EnvironmentLight::bilerp (environment_light.cpp:112-127) in numpy floats: the weights narrowed to
    float32, the blend in float32."""
    h, w = tex.shape[:2]
    f = np.float32
    right, v = math.floor(xx + 0.5), math.floor(yy + 0.5)  # lround of a non-negative value
    u1 = right - xx + .5
    if right == 0 or right == w:
        left, right = w - 1, 0
    else:
        left = right - 1
    if v == 0:
        v, v1 = 1, 1.0
    elif v == h:
        v, v1 = h - 1, 0.0
    else:
        v1 = v - yy + .5
    u0 = 1 - u1
    fu1, fu0, fv1, fv0 = f(u1), f(u0), f(v1), f(1 - v1)
    a = tex[v - 1, left] * fu1 + tex[v - 1, right] * fu0
    b = tex[v, left] * fu1 + tex[v, right] * fu0
    return a * fv1 + b * fv0


def env_lookup(tex, dirs):
    """EnvironmentLight::sample_dir (environment_light.cpp:146-148), one rounded operation at a time, acos
    and atan2 the host library's.  Pinned below against the unlensed restatement's frame."""
    h, w = tex.shape[:2]
    out = np.zeros((len(dirs), 3), np.float32)
    for i, dv in enumerate(dirs):
        r = 1. / math.sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2])
        ux, uy, uz = r * dv[0], r * dv[1], r * dv[2]
        theta, phi = math.acos(uy), math.atan2(-uz, ux) + PI
        out[i] = env_bilerp(tex, phi / 2. / PI * w, theta / PI * h)
    return out


class EnvSampler:
    """EnvironmentLight::init's tables and sample_L (environment_light.cpp:21-45, 130-144) in numpy: the
    sums sequential (cumsum), sin and cos the host library's."""

    def __init__(self, tex):
        self.tex = tex
        h, w = self.h, self.w = tex.shape[:2]
        f = np.float32
        il = (f(0.2126) * tex[..., 0] + f(0.7152) * tex[..., 1]) + f(0.0722) * tex[..., 2]
        s = np.array([math.sin(PI * (j + .5) / h) for j in range(h)])
        pdf = il.astype(np.float64) * s[:, None]
        self.pdf = pdf / np.cumsum(pdf.ravel())[-1]
        rows = np.cumsum(self.pdf, axis=1)[:, -1]
        with np.errstate(all="ignore"):
            self.conds = np.cumsum(self.pdf / rows[:, None], axis=1)
        self.marg = np.cumsum(rows)

    def sample(self, sx, sy):
        """(radiance float32 [3], wi [3], pdf float32) of the draws (sx, sy)."""
        y = min(int(np.searchsorted(self.marg, sy, side="right")), self.h - 1)
        x = min(int(np.searchsorted(self.conds[y], sx, side="right")), self.w - 1)
        phi, theta = x / self.w * 2.0 * PI, y / self.h * PI
        wi = [math.cos(phi - PI) * math.sin(theta), math.cos(theta), -math.sin(phi - PI) * math.sin(theta)]
        with np.errstate(all="ignore"):
            pdf = np.float32(np.float64(self.pdf[y, x] * self.w * self.h) / np.float64(2 * math.pi * math.pi * math.sin(theta)))
        return env_bilerp(self.tex, float(x), float(y)), wi, pdf


def frame_rays(camera_path, w, h):
    """The pixel-centre camera rays of a w x h frame (ro_camera_ray), row-major."""
    import ctypes as C
    cam = ol.load_camera(camera_path)
    cols = np.array(cam.c2w, np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(cam.pos, np.float64)
    o, d = np.zeros((h * w, 3)), np.zeros((h * w, 3))
    mn, mx = C.c_double(), C.c_double()
    for y in range(h):
        for x in range(w):
            ol.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, (x + 0.5) / w, (y + 0.5) / h,
                                   o[y * w + x], d[y * w + x], C.byref(mn), C.byref(mx))
    return o, d


def test_env_lookup_is_the_unlensed_restatements():
    """As tests/test_gpu_lensed_sky.py test_env_eval_is_the_reference_lookup: at ns_aa = 1, depth 0 a
    pixel whose camera ray hits nothing is sample_dir of that ray, so the unlensed restatement's frames
    (the closed room's and the open banana scene's) pin env_lookup on those pixels."""
    tex = np.ascontiguousarray(Case("env_bunny_96x72_s16").envmap, np.float32)
    seen = 0
    for name in ("env_bunny_96x72_s16", "banana_64x48_s16"):
        c = Case(name)
        bh = c.cfg["bh"]
        s = ol.Scene(c.scene_path)
        s.set_envmap(tex)
        p = ol.make_params(c.frame_w, c.frame_h, ns_aa=1, max_ray_depth=0, bh=bh)
        rgb, _, _, _ = ol.render(s, ol.load_camera(c.camera_path), p, 0, 0, c.frame_w, c.frame_h, threads=THREADS)
        o, d = frame_rays(c.camera_path, c.frame_w, c.frame_h)
        nohit = ol.ray_query(s, ol.make_params(1, 1, bh=bh), o, d)["status"] != HIT
        got = env_lookup(tex, d[nohit])
        assert np.array_equal(u32(got), u32(rgb.reshape(-1, 3)[nohit])), name
        assert len(np.unique(u32(got), axis=0)) >= 100
        seen += int(nohit.sum())
    assert seen >= 1000, seen  # 598 pixels of the closed room (test_env_eval_is_the_reference_lookup) and the open scene's sky


# ------------------------------------------------------------------ depth-0 frames
@pytest.mark.parametrize("lensed", [False, True])
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_disk_frame_at_depth_0(kerr, lensed):
    """test_gpu_disk.py test_frame_is_exact's pixel formulas, of the restatement: 96 x 72, ns_aa = 1,
    depth 0.  DISK: the checker's radiance of the crossing; HIT: the disk-less frame's pixel; any other:
    the sky rule in force -- the map along the unbent ray, or, lensed, along an ESCAPED ray's exit
    direction and black otherwise.  The camera records are checked like test_disk_queries'."""
    W, H = 96, 72
    case = Case(dc.CAMERA_CASE)
    cam = ol.load_camera(case.camera_path)
    k = dc.KERRS[kerr]
    scene = scene_of(SPHERES_L, env=True)
    tex = np.ascontiguousarray(Case("env_bunny_96x72_s16").envmap, np.float32)
    hole = dc.Hole(BH, k)
    disk = dc.Disk(hole, dc.isco(k[0]), dc.R_OUT, EM)
    o, d = frame_rays(case.camera_path, W, H)
    pq = ol.make_params(1, 1, bh=BH, kerr=k, disk=disk_of(kerr, dc.R_OUT), lensed_sky=lensed)
    rec = ol.ray_query(scene, pq, o, d)  # test_disk_queries checks every third of these both ways
    st = rec["status"]
    is_disk = st == DISK
    p0 =ol.make_params(W, H, ns_aa=1, max_ray_depth=0, bh=BH, kerr=k)
    rgb0, _, _, _ = ol.render(scene, cam, p0, 0, 0, W, H, threads=THREADS)
    p = ol.make_params(W, H, ns_aa=1, max_ray_depth=0, bh=BH, kerr=k, disk=disk_of(kerr, dc.R_OUT), lensed_sky=lensed)
    rgb, cnt, draws, ev = ol.render_events(scene, cam, p, 0, 0, W, H, threads=THREADS)
    assert (cnt == 1).all() and (draws == 0).all()
    px = rgb.reshape(-1, 3)
    exp = np.zeros_like(px)
    for i in np.flatnonzero(is_disk):
        c = dc.first_on(dc.crossings(hole, disk, o[i], d[i]))
        assert c is not None and c.row + 1 == int(rec["steps"][i]) and tc.same(rec["t"][i], c.t), i
        exp[i] = c.rgb
    hit = st == HIT
    exp[hit] = rgb0.reshape(-1, 3)[hit]
    if lensed:
        esc = st == ESCAPED
        exp[esc] = env_lookup(tex, rec["e"][esc])
        assert ((st == MISS) | (st == CAPTURED)).sum() >= 1
    else:
        sky = (st == MISS) | (st == CAPTURED)
        exp[sky] = env_lookup(tex, d[sky])
    n = {s: int((st == s).sum()) for s in (MISS, HIT, CAPTURED, ESCAPED, DISK)}
    print(f"{kerr} lensed={lensed}: miss / hit / captured / escaped / disk = {tuple(n.values())}")
    assert n[DISK] >= 300 and len(px) - n[DISK] >= 300
    bad = np.flatnonzero((u32(px) != u32(exp)).any(1))
    assert len(bad) == 0, (bad[:8], px[bad[:4]], exp[bad[:4]], st[bad[:4]])
    assert len(np.unique(u32(px[is_disk]), axis=0)) >= 100
    # the event counts: [0] the camera rays on the disk, [7] the escaped ones (lensed), nothing else
    e = ev.reshape(-1, ol.N_EVENTS)
    assert np.array_equal(e[:, 0], is_disk.astype(np.uint32))
    assert np.array_equal(e[:, 7], (st == ESCAPED).astype(np.uint32)) and not e[:, 1:7].any()


@pytest.mark.parametrize("metric", ["schwarzschild", "kerr"])
def test_lensed_frame_at_depth_0(metric):
    """test_gpu_lensed_sky.py test_lensed_frame_is_exact's pixel formulas, of the restatement: ESCAPED: the
    map along the exit direction; CAPTURED / MISS: black; a HIT whose record is the unflagged one: the
    unlensed frame's pixel.  The exit records are checked as in the exit-query tests."""
    kerr = FRAME_KERR if metric == "kerr" else None
    c = Case("banana_64x48_s16")
    W, H = c.frame_w, c.frame_h
    tex = np.ascontiguousarray(Case("env_bunny_96x72_s16").envmap, np.float32)
    s = ol.Scene(c.scene_path)
    s.set_envmap(tex)
    cam = ol.load_camera(c.camera_path)
    o, d = frame_rays(c.camera_path, W, H)
    un = ol.ray_query(s, ol.make_params(1, 1, bh=FRAME_BH, kerr=kerr), o, d)
    fl = ol.ray_query(s, ol.make_params(1, 1, bh=FRAME_BH, kerr=kerr, lensed_sky=True), o, d)
    st = fl["status"]
    if kerr is None:
        want = xc.expected_exit_records(xc.Chains(FRAME_BH, o, d), hit_records(un))
        assert_same_records(fl, want, metric)
    else:
        max_steps = 4 * tc.steps_of(FRAME_BH[4])
        for i in np.flatnonzero(st == ESCAPED):
            row = xc.kerr_exit_row(FRAME_BH, kerr, o[i], d[i], int(fl[i]["steps"]), max_steps)
            assert row is not None and tc.same(fl[i]["e"], -row[1]), i
    n = {k: int((st == k).sum()) for k in (MISS, HIT, CAPTURED, ESCAPED)}
    print(f"{metric}: miss / hit / captured / escaped = {tuple(n.values())}")
    assert n[ESCAPED] >= 50 and n[CAPTURED] >= 50 and n[HIT] >= 400, n
    rgb, cnt, _, ev = ol.render_events(s, cam, ol.make_params(W, H, ns_aa=1, max_ray_depth=0, bh=FRAME_BH, kerr=kerr, lensed_sky=True),
                                       0, 0, W, H, threads=THREADS)
    rgb0, cnt0, _, _ = ol.render(s, cam, ol.make_params(W, H, ns_aa=1, max_ray_depth=0, bh=FRAME_BH, kerr=kerr), 0, 0, W, H,
                                 threads=THREADS)
    assert (cnt == 1).all() and (cnt0 == 1).all()
    px, px0 = rgb.reshape(-1, 3), rgb0.reshape(-1, 3)
    esc = st == ESCAPED
    sky = env_lookup(tex, fl["e"][esc])
    assert np.array_equal(u32(px[esc]), u32(sky)) and len(np.unique(u32(sky), axis=0)) >= 100
    assert not u32(px[(st == CAPTURED) | (st == MISS)]).any()
    same = (st == HIT) & np.array([fl[i].tobytes() == un[i].tobytes() for i in range(len(fl))])
    assert same.sum() >= 400 and np.array_equal(u32(px[same]), u32(px0[same]))
    assert u32(px0[st == CAPTURED]).any() and not np.array_equal(u32(px[esc]), u32(px0[esc]))
    assert np.array_equal(ev.reshape(-1, ol.N_EVENTS)[:, 7], esc.astype(np.uint32))


# ------------------------------------------------------------------ the integrator's rules, pixel by pixel
def coord(n, v):
    """(to_local(v), to_world(v)) in the shading frame of normal n (the restated make_coord_space)."""
    o2w, a, b = np.zeros(9), np.zeros(3), np.zeros(3)
    ol.lib().ro_coord_space(np.ascontiguousarray(n, np.float64), np.ascontiguousarray(v, np.float64), o2w, a, b)
    return a, b


def test_lensed_environment_sample_takes_the_map_along_the_exit_direction():
    """DESIGN.md §11, direct_importance's lensed branch, at ns_aa = 1, depth 1, ns_area_light = 1 on the
    lensed Kerr frame.  The flag changes one term of a hit pixel: the environment light's sample E, last
    in the light list -- E_u = sample x f x cos / pdf if the unlensed shadow query finds nothing, E_l =
    map(exit direction) x f x cos / pdf if the lensed one escapes -- with the same draws, direction and
    pdf.  So (pixel_l - pixel_u) x n_samples = E_l - E_u, E from EnvSampler's own tables, the checked exit
    record of the shadow ray and env_lookup; to 1e-5 of the pixels (two float32 sums of three terms)."""
    c = Case("banana_64x48_s16")
    W, H = c.frame_w, c.frame_h
    tex = np.ascontiguousarray(Case("env_bunny_96x72_s16").envmap, np.float32)
    s = ol.Scene(c.scene_path)
    s.set_envmap(tex)
    cam = ol.load_camera(c.camera_path)
    sf = rrt.SceneFile(c.scene_path)
    bsdfs = lc.bsdfs_of(sf)
    desc = rrt.SceneDesc.from_address(sf.desc())
    assert all(desc.lights[i].type in (2, 3) for i in range(desc.n_lights))  # directional, infinite hemisphere
    first = sum(0 if desc.lights[i].is_delta else 2 for i in range(desc.n_lights))  # the listed lights' draws
    total = desc.n_lights + 1
    kw = dict(ns_aa=1, max_ray_depth=1, ns_area_light=1, bh=FRAME_BH, kerr=FRAME_KERR)
    pu, _, du, _ = ol.render(s, cam, ol.make_params(W, H, **kw), 0, 0, W, H, threads=THREADS)
    pl, _, dl, ev = ol.render_events(s, cam, ol.make_params(W, H, lensed_sky=True, **kw), 0, 0, W, H, threads=THREADS)
    q_u = ol.make_params(1, 1, bh=FRAME_BH, kerr=FRAME_KERR)
    q_l = ol.make_params(1, 1, bh=FRAME_BH, kerr=FRAME_KERR, lensed_sky=True)
    o, d = frame_rays(c.camera_path, W, H)
    rec = ol.ray_query(s, q_u, o, d)
    sampler = EnvSampler(tex)
    n = {"pixels": 0, "behind": 0, "escaped": 0, "moved": 0}
    for i in np.flatnonzero(rec["status"] == HIT):
        x, y = int(i % W), int(i // W)
        assert bsdfs[int(rec["bsdf"][i])][0] == lc.DIFFUSE and du[y, x] == dl[y, x] == first + 2
        key = ol.lib().ro_pixel_key(0, x, y)
        sy = ol.lib().ro_keyed_rand(key, first) / lc.RAND_MAX  # the grid sampler draws y first
        sx = ol.lib().ro_keyed_rand(key, first + 1) / lc.RAND_MAX
        rad, wi, pdf = sampler.sample(sx, sy)
        cos = lc.to_local_z(rec["n"][i], wi)
        n["pixels"] += 1
        E_l = E_u = np.zeros(3)
        escaped = False
        if cos < 0:
            n["behind"] += 1
        else:
            so = [float(rec["hit_p"][i][k]) + lc.EPS * wi[k] for k in range(3)]
            f = lc.diffuse_f(bsdfs[int(rec["bsdf"][i])][1])
            sh = ol.ray_query(s, q_l, [so], [wi], any_hit=True)[0]  # test_exit_queries_kerr checks such records
            escaped = int(sh["status"]) == ESCAPED
            with np.errstate(all="ignore"):
                if escaped:
                    E_l = (((env_lookup(tex, [sh["e"]])[0] * f) * np.float32(cos)) / pdf).astype(np.float64)
                if not ol.shadow_query(s, q_u, so, wi):
                    E_u = (((rad * f) * np.float32(cos)) / pdf).astype(np.float64)
        assert ev[y, x, 6] == int(escaped), (x, y)
        n["escaped"] += escaped
        got = (pl[y, x].astype(np.float64) - pu[y, x]) * total
        want = E_l - E_u
        tol = 1e-5 * (np.abs(pl[y, x]).max() + np.abs(pu[y, x]).max()) * total + 1e-9
        assert np.isfinite(want).all() and np.abs(got - want).max() <= tol, (x, y, got, want, E_l, E_u)
        n["moved"] += bool(np.abs(want).max() > 100 * tol)
    print(n)
    # measured: 981 hit pixels, 520 samples behind the surface, 360 escaped, 104 with |E_l - E_u| > 100 tol
    assert n["pixels"] >= 400 and n["escaped"] >= 100 and n["moved"] >= 50, n


@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_mirror_bounce_onto_the_disk_at_depth_2(kerr):
    """DESIGN.md §12, at_least_one_bounce's disk branch at a delta level: ns_aa = 1, depth 2, CBspheres
    through the wide camera.  A camera ray on the mirror sphere takes no direct light and no draw; its one
    bounce ray is the reflection of the hitting chord.  Where that ray's checked record is a DISK record
    the pixel is ((rgb x (reflectance / |cos|)) x |cos| / 1) / 0.7f in float32, rgb the checker's radiance
    of the crossing: the disk's emission through the delta level's term, and nothing from a child level."""
    W, H = lc.W, lc.H
    k = dc.KERRS[kerr]
    path = os.path.join(GOLD, "scenes", "CBspheres.rrts")
    scene = scene_of(path)
    bsdfs = lc.bsdfs_of(rrt.SceneFile(path))
    mirror = [i for i, (t, _) in enumerate(bsdfs) if t == 2]  # RRT_BSDF_MIRROR
    assert len(mirror) == 1
    refl = bsdfs[mirror[0]][1][:3].astype(np.float32)
    cam_path = Case(lc.WIDE_CASE).camera_path
    hole = dc.Hole(BH, k)
    disk = dc.Disk(hole, dc.isco(k[0]), dc.R_OUT, EM)
    xs, ys = lc.frame_pixels(1)
    o, d = lc.camera_rays(cam_path, xs, ys)
    q_un = ol.make_params(1, 1, bh=BH, kerr=k)
    q_dk = ol.make_params(1, 1, bh=BH, kerr=k, disk=disk_of(kerr, dc.R_OUT))
    cam_rec = ol.ray_query(scene, q_dk, o, d)
    p = ol.make_params(W, H, ns_aa=1, max_ray_depth=2, ns_area_light=1, bh=BH, kerr=k, disk=disk_of(kerr, dc.R_OUT))
    rgb, cnt, draws, ev = ol.render_events(scene, ol.load_camera(cam_path), p, 0, 0, W, H, threads=THREADS)
    f = np.float32
    n = {"mirror": 0, "disk": 0}
    for i in np.flatnonzero((cam_rec["status"] == HIT) & (cam_rec["bsdf"] == mirror[0])):
        x, y = int(xs[i]), int(ys[i])
        un = hit_records(ol.ray_query(scene, q_un, o[i:i + 1], d[i:i + 1]))[0]
        want, _ = dc.expected_record(hole, disk, o[i], d[i], un)  # the camera record, by the checker
        assert int(want["status"]) == HIT and tc.same(want["hit_p"], cam_rec["hit_p"][i]) and tc.same(want["n"], cam_rec["n"][i])
        steps = int(cam_rec["steps"][i])
        rows, _ = ol.kerr_chain(BH, k[0], k[1], o[i], d[i], max_rows=steps)
        wo, _ = coord(cam_rec["n"][i], -rows[steps - 1, 3:6])
        wi_l = [-wo[0], -wo[1], wo[2]]
        _, wi = coord(cam_rec["n"][i], wi_l)
        o2 = np.array([float(cam_rec["hit_p"][i][j]) + lc.EPS * wi[j] for j in range(3)])
        un2 = hit_records(ol.ray_query(scene, q_un, [o2], [wi]))[0]
        rec2, _ = dc.expected_record(hole, disk, o2, wi, un2)
        n["mirror"] += 1
        assert cnt[y, x] == 1
        if int(rec2["status"]) != DISK:
            assert ev[y, x, 3] == 0, (x, y)
            continue
        n["disk"] += 1
        c = dc.first_on(dc.crossings(hole, disk, o2, wi))
        az = f(abs(wi_l[2]))
        px = (((c.rgb * (refl / az)) * az) / f(1.0)) / f(0.7)
        assert ev[y, x, 3] == 1 and not ev[y, x, [0, 1, 2, 4, 5, 6, 7]].any() and draws[y, x] == 0, (x, y, ev[y, x])
        assert np.array_equal(u32(rgb[y, x]), u32(px)), (x, y, rgb[y, x], px)
    print(f"{kerr}: {n}")
    assert n["mirror"] >= 100 and n["disk"] >= 32, n


# ------------------------------------------------------------------ depth 1 with the light flag
@pytest.mark.parametrize("kerr", sorted(dc.KERRS))
def test_light_flag_adds_the_checkers_term_at_depth_1(kerr):
    """tests/test_gpu_disk_light.py's identity, of the restatement: ns_aa = 1, depth 1, ns_area_light = 4,
    through the wide camera; on every checked pixel of disk_light_check's pixel set
    on == float32(off + D) per channel, D the checker's disk term from the pixel's keyed draws and the
    crossings its shadow rays end on, and the draws grow by 2 ns_area_light."""
    why = lc.parity()
    if why:
        pytest.skip("PARITY PRECONDITION NOT MET: " + why)
    W, H, NS = lc.W, lc.H, lc.NS_AREA_LIGHT
    k = dc.KERRS[kerr]
    scene = scene_of(SPHERES_L)
    cam_path = Case(lc.WIDE_CASE).camera_path
    cam = ol.load_camera(cam_path)
    hole = dc.Hole(BH, k)
    disk = dc.Disk(hole, dc.isco(k[0]), dc.R_OUT, EM)
    light = lc.Light(hole, disk)
    sf = rrt.SceneFile(SPHERES_L)
    bsdfs = lc.bsdfs_of(sf)
    first_draw = lc.n_listed_draws(sf, NS)
    xs, ys = lc.frame_pixels()
    o, d = lc.camera_rays(cam_path, xs, ys)
    p_un = ol.make_params(1, 1, bh=BH, kerr=k)
    cam_rec, _ = dc.expected_records(hole, disk, o, d, hit_records(ol.ray_query(scene, p_un, o, d)))
    px = []
    for i in np.flatnonzero(cam_rec["status"] == HIT):
        if not lc.checkable(bsdfs, int(cam_rec["bsdf"][i]), cam_rec["n"][i]):
            continue
        key = ol.lib().ro_pixel_key(0, int(xs[i]), int(ys[i]))
        px.append((int(xs[i]), int(ys[i]), lc.diffuse_f(bsdfs[int(cam_rec["bsdf"][i])][1]),
                   lc.pixel_samples(light, cam_rec["hit_p"][i], cam_rec["n"][i], key, first_draw, NS)))
    rays = [s for _, _, _, ss in px for s in ss if s.shadow]
    so, sd = np.array([s.o for s in rays]), np.array([s.wi for s in rays])
    sun = hit_records(ol.ray_query(scene, p_un, so, sd))
    ends = []
    for j, s in enumerate(rays):
        s.crossing, _, status = lc.shadow_crossing(hole, disk, so[j], sd[j], sun[j])
        ends.append(status)
    n_disk, n_stopped = ends.count(DISK), ends.count(HIT) + ends.count(CAPTURED)
    print(f"{kerr}: {len(px)} checked pixels, {len(rays)} shadow rays: {n_disk} end on the disk, {n_stopped} stopped")
    assert len(px) >= 300 and n_disk >= 200 and n_stopped >= 50
    kw = dict(ns_aa=1, max_ray_depth=1, ns_area_light=NS, bh=BH, kerr=k)
    off, cnt_off, draws_off, _ = ol.render(scene, cam, ol.make_params(W, H, disk=disk_of(kerr, dc.R_OUT), **kw), 0, 0, W, H, threads=THREADS)
    on, cnt_on, draws_on, ev = ol.render_events(scene, cam, ol.make_params(W, H, disk=disk_of(kerr, dc.R_OUT, light=True), **kw),
                                                0, 0, W, H, threads=THREADS)
    assert (cnt_on == 1).all() and (cnt_off == 1).all()
    bad, lit, terms = [], 0, []
    for x, y, f, samples in px:
        assert draws_off[y, x] == first_draw and draws_on[y, x] == first_draw + 2 * NS
        rgbs = [s.crossing.rgb if s.shadow and s.crossing is not None else None for s in samples]
        D = lc.pixel_term(samples, rgbs, f)
        assert ev[y, x, 5] == sum(r is not None for r in rgbs)
        want = off[y, x] + D
        terms.append(D)
        lit += bool(D.any())
        if not (u32(on[y, x]) == u32(want)).all():
            bad.append((x, y, on[y, x], want, off[y, x], D))
    assert not bad, (len(bad), bad[:4])
    assert lit >= 100 and len(np.unique(u32(np.array(terms)), axis=0)) >= 100
    # every pixel: the flag adds 2 NS draws where direct light is taken, none elsewhere
    lit_px = draws_off > 0
    assert np.array_equal(draws_on.astype(np.int64) - draws_off, np.where(lit_px, 2 * NS, 0))


# ------------------------------------------------------------------ what the disk leaves alone
@pytest.mark.parametrize("depth", [1, 3])
def test_pixels_without_an_event_are_the_diskless_pixels(depth):
    """At R_OUT = 16 M the escape radius does not move.  There every pixel whose eight event counts are all
    zero -- no ray of it met the disk, none escaped -- is the disk-less Kerr restatement's pixel bit for
    bit: rgb, sample count and draws (tests/test_gpu_kerr.py pins that frame's march and integrator)."""
    W, H = 96, 72
    kerr = "a0.9"
    k = dc.KERRS[kerr]
    scene = scene_of(os.path.join(GOLD, "scenes", "CBspheres.rrts"))
    hole = dc.Hole(BH, k)
    assert (dc.R_OUT * hole.m) ** 2 + hole.a2 < root_esc2(scene, hole)
    cam = ol.load_camera(Case(lc.WIDE_CASE).camera_path)
    kw = dict(ns_aa=4, max_ray_depth=depth, ns_area_light=2, bh=BH, kerr=k)
    a = ol.render(scene, cam, ol.make_params(W, H, **kw), 0, 0, W, H, threads=THREADS)
    b = ol.render_events(scene, cam, ol.make_params(W, H, disk=disk_of(kerr, dc.R_OUT), **kw), 0, 0, W, H, threads=THREADS)
    clean = ~b[3].any(-1)
    print(f"depth {depth}: {int(clean.sum())} of {W * H} pixels without an event; events {b[3].reshape(-1, 8).sum(0)}")
    assert clean.sum() >= 300 and (~clean).sum() >= 300
    assert np.array_equal(u32(a[0][clean]), u32(b[0][clean]))
    assert np.array_equal(a[1][clean], b[1][clean]) and np.array_equal(a[2][clean], b[2][clean])
    # and the disk does something elsewhere
    assert not np.array_equal(u32(a[0][~clean]), u32(b[0][~clean]))
