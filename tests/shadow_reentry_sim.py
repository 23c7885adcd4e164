"""numpy mirror of the shadow-ray occlusion proof with the re-entry rule (rrt_proof.h occ_exit,
KParams::shadow_reentry): tests/shadow_proof_sim.py's run, except that a segment whose
end has left the root box without a certain crossing no longer ends the proof.

TEST INFRASTRUCTURE ONLY (tests/test_shadow_reentry.py, tools/proof_sweep.py --shadow-mirror reentry):
the product runs the HIP version.

A ray that passes within a few r_s of the hole is thrown out through the room's open side; a few
rows later the reference's recurrence changes the sign of v and the next chord comes back through
the room and crosses a wall.  The recurrence, the cancelling-step test, the capture-sphere test and
the margin are the ones of every other row; a segment with both ends beyond the same face of the root
box meets no kept triangle (every primitive lies inside the root box): the face test's plane test
rejects it.
"""
import numpy as np

from miss_proof_sim import ETA, _step0, rec_cancels, rec_hole_farther, rec_point, rec_row, rec_turn
from shadow_proof_sim import _face


def _exit(faces, box, K, a, b, m, reentry):
    """occ_exit for one ray (a or b outside the trigger box): (1 | 0 | -1, triangle index, b outside
    the root box)."""
    lo, hi = box
    out = False
    for k in range(3):
        for f, past in ((k, not (b[k] >= lo[k] and a[k] >= lo[k])), (k + 3, not (b[k] <= hi[k] and a[k] <= hi[k]))):
            if past:
                idx = _face(faces[f], a, b, m)
                if idx >= 0:
                    return 1, idx, False
        out = out or not (K["lo"][k] <= b[k] <= K["hi"][k])
    return (-1 if out and not reentry else 0), -1, out


def run(K, faces, box, o, d, ms=1.0, reentry=True):
    """The proof for rays (o, d).  Returns (proven [n], step [n], triangle [n], points [steps+1, n, 3]
    of the recurrence (NaN once a ray's proof ended), margins [steps+1, n], left [n]: the row at
    which a segment end first lay outside the root box without a certain crossing, or -1).
    reentry=False: tests/shadow_proof_sim.py run, statement for statement."""
    n = len(o)
    steps = K["steps"]
    X, Y, u0, up0, _, _ = _step0(K, o, d)
    pts = np.full((steps + 1, n, 3), np.nan)
    mrg = np.full((steps + 1, n), np.nan)
    proven = np.zeros(n, bool)
    step = np.full(n, -1)
    tri = np.full(n, -1)
    left = np.full(n, -1)
    alive = np.ones(n, bool)
    pts[0] = o
    vprev = K["rho"] * u0
    s = u0 * K["co1"] - up0 * K["si"] / K["rho"]
    ea = np.ones(n)
    eb = np.zeros(n)
    sig = np.ones(n)
    rp = 1.0 / u0
    a_in = np.all(o >= box[0], 1) & np.all(o <= box[1], 1)
    rc = K["r"] * (1.0 + 1e-9)
    with np.errstate(all="ignore"):
        for j in range(steps):
            sg = np.where(vprev < 0.0, -1.0, 1.0)
            up, s, v = rec_row(K, vprev, s)
            alive &= ~rec_cancels(K, s, up, v)
            na, nb, sig = rec_turn(K, sg, sig, ea, eb)
            r = K["rho"] / np.abs(v) * (1.0 + 1e-6)
            m = ms * ETA * (np.maximum(rp, r) + K["scale"])
            rb = rc + m
            alive &= rec_hole_farther(K, vprev, v, rb * rb)
            pa = rec_point(K, X, Y, ea, eb, vprev)
            pb = rec_point(K, X, Y, na, nb, v)
            pts[j + 1] = np.where(alive[:, None], pb, np.nan)
            mrg[j + 1] = np.where(alive, m, np.nan)
            b_in = np.all(pb >= box[0], 1) & np.all(pb <= box[1], 1)
            for i in np.nonzero(alive & ~(b_in & a_in))[0]:
                res, idx, out = _exit(faces, box, K, pa[i], pb[i], m[i], reentry)
                if out and left[i] < 0:
                    left[i] = j
                if res:
                    alive[i] = False
                    proven[i], step[i], tri[i] = res > 0, j, idx
            a_in = b_in
            rp, vprev, ea, eb = r, v, na, nb
    return proven, step, tri, pts, mrg, left


def surface_rays(T, lights, n, g, eps=1e-11):
    """Shadow rays from n random surface points (by area) of the triangles T towards random points of
    the scene's area / point lights, as tests/proof_sweep.py check_shadow draws them: (o [n, 3],
    d [n, 3]), or None when the scene has no such light."""
    ls = [lv for ty, _, lv in lights if ty in (0, 1)]
    kind = [ty for ty, _, _ in lights if ty in (0, 1)]
    if not ls:
        return None
    area = 0.5 * np.linalg.norm(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]), axis=1)
    t = g.choice(len(T), n, p=area / area.sum())
    u, v = g.random(n), g.random(n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    hp = T[t, 0] + u[:, None] * (T[t, 1] - T[t, 0]) + v[:, None] * (T[t, 2] - T[t, 0])
    li = g.integers(0, len(ls), n)
    pos = np.array([ls[i][0] for i in li])
    isarea = np.array([kind[i] == 0 for i in li])[:, None]
    dx = np.where(isarea, np.array([ls[i][2] for i in li]), 0.0)
    dy = np.where(isarea, np.array([ls[i][3] for i in li]), 0.0)
    p = pos + (g.random(n) - 0.5)[:, None] * dx + (g.random(n) - 0.5)[:, None] * dy
    wi = p - hp
    wi /= np.linalg.norm(wi, axis=1)[:, None]
    return hp + eps * wi, wi


def compare(K, faces, box, T, o, d, rows, nrow):
    """The proof with and without the rule on rays (o, d) whose reference chains are rows [n, steps+1, 8]
    / nrow [n] (oracle ro_micro_chain).  Returns a dict: rays, proven_before, proven_after,
    proven_after_leaving, rows_after_leaving (of those rays: rows between leaving and the crossing),
    worst_dev_over_margin (every row the new proof ran, rows after leaving included), violations
    (proven rays whose reference chain is captured or ends by the proof's segment, or whose reference
    triangle test rejects that segment against the proof's triangle), lost (rays the old rule proves
    that the new one does not prove at the same row and triangle), proven [n] (the new rule's)."""
    import ctypes as C

    import oracle_lib as O
    from shadow_proof_sim import run as run_old

    p0, s0, t0, _, _ = run_old(K, faces, box, o, d)
    p1, s1, t1, pts, mrg, left = run(K, faces, box, o, d)
    worst = 0.0
    for k in range(1, K["steps"] + 1):
        ok = (nrow > k) & np.isfinite(mrg[k])
        if ok.any():
            dev = np.linalg.norm(pts[k][ok] - rows[ok, k, 0:3], axis=1) / mrg[k][ok]
            worst = max(worst, float(dev.max()))
    hit_p, nrm, zero_n = np.zeros(3), np.zeros(3), np.zeros(9)
    bad = []
    for i in np.nonzero(p1)[0]:
        k = s1[i]
        if not (nrow[i] > k and not rows[i, :k + 1, 7].any()):
            bad.append((int(i), int(k), "captured or ended"))
            continue
        mt = C.c_double(rows[i, k, 6])
        if O.lib().ro_tri_intersect(T[t1[i]].ravel().copy(), zero_n, rows[i, k, 0:3].copy(), rows[i, k, 3:6].copy(),
                                    C.byref(mt), hit_p, nrm) != 1:
            bad.append((int(i), int(k), "triangle test"))
    lost = np.nonzero(p0 & ~(p1 & (s1 == s0) & (t1 == t0)))[0]
    after = p1 & (left >= 0)
    return {"rays": len(o), "proven_before": int(p0.sum()), "proven_after": int(p1.sum()),
            "proven_after_leaving": int(after.sum()),
            "rows_after_leaving": sorted(int(v) for v in (s1 - left)[after]),
            "worst_dev_over_margin": worst, "violations": bad, "lost": [int(i) for i in lost], "proven": p1}


def check_config(cfg, n, g):
    """tests/proof_sweep.py check_shadow with both rules on one configuration (scene file sf, root box
    lo / hi, hole bh): compare()'s counts, violations as a number."""
    from miss_proof_sim import constants
    from proof_sweep import _chains
    from shadow_proof_sim import occluders, trigger_box

    empty = {"rays": 0, "proven_before": 0, "proven_after": 0, "proven_after_leaving": 0,
             "worst_dev_over_margin": 0.0, "violations": 0, "lost": 0}
    K = constants(cfg["bh"], cfg["lo"], cfg["hi"])
    T = cfg["sf"].triangles()
    faces, w = occluders(T, cfg["lo"], cfg["hi"])
    if not any(len(f) for f in faces):
        return empty
    od = surface_rays(T, cfg["sf"].lights(), n, g)
    if od is None:
        return empty
    rows, nrow = _chains(cfg["bh"], od[0], od[1], K["steps"])
    r = compare(K, faces, trigger_box(K, w), T, od[0], od[1], rows, nrow)
    return {"rays": r["rays"], "proven_before": r["proven_before"], "proven_after": r["proven_after"],
            "proven_after_leaving": r["proven_after_leaving"], "worst_dev_over_margin": r["worst_dev_over_margin"],
            "violations": len(r["violations"]), "lost": len(r["lost"])}
