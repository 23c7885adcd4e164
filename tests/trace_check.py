"""The exact checker of the ray queries (rrt_trace_rays / rrt_trace_camera, include/rrt.h) -- all of
it CPU restatement (oracle/restate through oracle_lib) -- and the ray sets the tests share.

For every ray, oracle_lib.query gives (hit, hit_p, n, bsdf): status == HIT iff hit, and hit_p, n
and bsdf must match bit for bit.  For a hit, row steps - 1 of the micro-ray chain (ro_micro_chain,
or ro_kerr_chain for Kerr) is the segment (o, d, max_t) that hit: w_out must be -d of that row, and
the restated primitive test (ro_tri_intersect / ro_sphere_intersect) of primitive `prim` ALONE on
that segment must accept, reproduce hit_p and n bit for bit and leave t in max_t; prim's object
must carry bsdf.  Without a hit: CAPTURED iff row steps - 1 is the chain's first row with the
capture flag, else MISS with no capture flag in rows < steps (Schwarzschild: steps = all of the
march; Kerr: steps >= 1, the restated chain has no escape cutoff).
"""
import ctypes as C

import numpy as np

import oracle_lib as ol
import rrt

MISS, HIT, CAPTURED = rrt.RRT_RAY_MISS, rrt.RRT_RAY_HIT, rrt.RRT_RAY_CAPTURED
DEFAULT_BH = (0.0, 1.0, 0.0, 0.1, 0.1)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def ray_sets(n=512, seed=7):
    """The four ray sets, draws in this order from default_rng(seed): {name: (o [n, 3], d [n, 3])}."""
    g = np.random.default_rng(seed)
    lo, hi, c = np.array([-1.0, 0.0, -1.0]), np.array([1.0, 1.5, 1.0]), np.array([0.0, 1.0, 0.0])
    O = lo + (hi - lo) * g.random((n, 3))
    T = c + 0.05 * g.normal(size=(n, 3))
    U = unit(g.normal(size=(n, 3)))
    V = unit(U + 0.3 * g.normal(size=(n, 3)))
    W = unit(-U + 0.15 * g.normal(size=(n, 3)))
    R = unit(g.normal(size=(n, 3)))
    far = c + 5 * U
    return {"interior": (O, R), "aimed": (O, unit(T - O)), "outward": (far, V), "inward": (far, W)}


def steps_of(dtheta):
    j = 0
    while j * dtheta < 2 * np.pi:  # bvh.cpp:105
        j += 1
    return j


class Prims:
    """Geometry, normals and bsdf per build-order primitive, from SceneFile.desc(): objects in
    order, a mesh's triangles in index order, a sphere as one primitive."""

    def __init__(self, scene_file):
        d = rrt.SceneDesc.from_address(scene_file.desc())
        self.items = []  # ("tri", p9, n9, bsdf) | ("sphere", c3, r, bsdf)
        for i in range(d.n_objects):
            o = d.objects[i]
            if o.kind == 0:
                if o.n_triangles == 0:
                    continue
                P = np.ctypeslib.as_array(o.positions, shape=(o.n_vertices * 3,)).reshape(-1, 3)
                N = np.ctypeslib.as_array(o.normals, shape=(o.n_vertices * 3,)).reshape(-1, 3)
                idx = np.ctypeslib.as_array(o.indices, shape=(o.n_triangles * 3,)).reshape(-1, 3)
                for t in idx:
                    self.items.append(("tri", P[t].ravel().copy(), N[t].ravel().copy(), int(o.bsdf)))
            else:
                self.items.append(("sphere", np.array(o.center, np.float64), float(o.radius), int(o.bsdf)))

    def __len__(self):
        return len(self.items)

    def intersect(self, k, o, d, max_t):
        """The restated primitive test of primitive k alone on the segment (o, d, max_t):
        (accepted, max_t afterwards, hit_p, n)."""
        it = self.items[k]
        mt = C.c_double(max_t)
        hp, nn = np.zeros(3), np.zeros(3)
        o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
        if it[0] == "tri":
            ok = ol.lib().ro_tri_intersect(it[1], it[2], o, d, C.byref(mt), hp, nn)
        else:
            ok = ol.lib().ro_sphere_intersect(it[1], it[2], o, d, C.byref(mt), hp, nn, 1)
        return bool(ok), mt.value, hp, nn

    def bsdf(self, k):
        return self.items[k][3]


class Oracle:
    """The restatement's answers for rays under one spacetime: bh = (cx, cy, cz, r_s, dtheta),
    kerr = None or (spin, axis)."""

    def __init__(self, scene_path, bh=DEFAULT_BH, kerr=None):
        self.scene = ol.Scene(scene_path)
        self.bh, self.kerr = tuple(bh), kerr
        self.params = ol.make_params(1, 1, bh=self.bh, kerr=kerr)
        self.n_steps = steps_of(self.bh[4])

    def query(self, o, d):
        """[(hit, hit_p, n, bsdf)] per ray (computed once per ray set: callers keep the list)."""
        return [ol.query(self.scene, self.params, o[i], d[i]) for i in range(len(o))]

    def chain(self, o, d, rows):
        """The first `rows` rows (o3, d3, max_t, captured) of the ray's micro-ray chain (fewer if
        it is captured earlier: the chain ends with the first captured row)."""
        rows = max(int(rows), 1)
        if self.kerr is None:
            out = np.zeros((rows, 8))
            n = ol.lib().ro_micro_chain(np.array(self.bh, np.float64), np.ascontiguousarray(o, np.float64),
                                        np.ascontiguousarray(d, np.float64), out, rows)
            return out[:n]
        ch, _ = ol.kerr_chain(self.bh, self.kerr[0], self.kerr[1], o, d, max_rows=rows)
        return ch[:, :8]


def restatement_counts(orc, o, d, answers):
    """(hit, captured, miss) of the rays as the restatement alone sees them."""
    counts = [0, 0, 0]
    for i in range(len(o)):
        if answers[i][0]:
            counts[0] += 1
        elif orc.kerr is None:
            counts[1 if orc.chain(o[i], d[i], orc.n_steps)[-1, 7] else 2] += 1
    return tuple(counts)


def check_closest(orc, prims, o, d, answers, hits):
    """Every field of the closest-hit records `hits` (HIT_DTYPE [n]) of the rays (o, d) against the
    restatement (answers = orc.query(o, d)).  Returns (hit, captured, miss) counts."""
    assert len(hits) == len(o)
    counts = [0, 0, 0]
    for i in range(len(o)):
        h = hits[i]
        hit, hp, nn, bsdf = answers[i]
        st, steps = int(h["status"]), int(h["steps"])
        where = f"ray {i}: status {st} steps {steps}"
        assert (st == HIT) == hit, where
        assert steps >= 1, where
        ch = orc.chain(o[i], d[i], steps)
        if hit:
            counts[0] += 1
            assert same(h["hit_p"], hp) and same(h["n"], nn) and int(h["bsdf"]) == bsdf, where
            assert len(ch) >= steps and not ch[:steps, 7].any(), where  # no capture up to the segment
            row = ch[steps - 1]
            assert same(h["w_out"], -row[3:6]), where
            k = int(h["prim"])
            assert 0 <= k < len(prims), where
            ok, mt, php, pn = prims.intersect(k, row[0:3], row[3:6], row[6])
            assert ok and same(php, h["hit_p"]) and same(pn, h["n"]) and same(mt, h["t"]), where
            assert prims.bsdf(k) == int(h["bsdf"]), where
            continue
        assert st in (MISS, CAPTURED), where
        assert not bits(np.concatenate([h["hit_p"], h["n"], h["w_out"], [h["t"]]])).any(), where
        assert int(h["prim"]) == -1 and int(h["bsdf"]) == -1, where
        first_cap = len(ch) == steps and bool(ch[steps - 1, 7]) and not ch[:steps - 1, 7].any()
        if st == CAPTURED:
            counts[1] += 1
            assert first_cap, where
        else:
            counts[2] += 1
            assert not ch[:steps, 7].any(), where
            if orc.kerr is None:
                assert steps == orc.n_steps, where  # all marched
    return tuple(counts)


def check_any(closest, any_hits):
    """The shadow query's records against the (checked) closest-hit records of the same rays:
    status and steps equal, every hit field 0 / -1."""
    assert len(closest) == len(any_hits)
    assert np.array_equal(closest["status"], any_hits["status"])
    assert np.array_equal(closest["steps"], any_hits["steps"])
    for f in ("hit_p", "n", "w_out", "t"):
        assert not bits(any_hits[f]).any(), f
    assert (any_hits["prim"] == -1).all() and (any_hits["bsdf"] == -1).all()


def brute_force_records(orc, prims, o, d, answers):
    """Records built from the restatement alone: for every hit a search over (segment, primitive)
    for the pair whose single-primitive test reproduces ro_query's bits; the capture / miss rows
    from the chain.  The search must succeed for every hit (the single-primitive check is sound)."""
    out = np.zeros(len(o), rrt.HIT_DTYPE)
    out["prim"], out["bsdf"] = -1, -1
    for i in range(len(o)):
        hit, hp, nn, bsdf = answers[i]
        ch = orc.chain(o[i], d[i], orc.n_steps)
        if not hit:
            cap = bool(ch[-1, 7])
            out[i]["status"] = CAPTURED if cap else MISS
            out[i]["steps"] = len(ch) if cap else orc.n_steps
            continue
        found = None
        for s, row in enumerate(ch):
            if row[7]:
                break
            for k in range(len(prims)):
                ok, mt, php, pn = prims.intersect(k, row[0:3], row[3:6], row[6])
                if ok and same(php, hp) and same(pn, nn) and prims.bsdf(k) == bsdf:
                    found = (s, k, mt, row)
                    break
            if found:
                break
        assert found, f"ray {i}: no (segment, primitive) pair reproduces the query's hit"
        s, k, mt, row = found
        r = out[i]
        r["status"], r["steps"], r["prim"], r["bsdf"], r["t"] = HIT, s + 1, k, bsdf, mt
        r["hit_p"], r["n"], r["w_out"] = hp, nn, -row[3:6]
    return out
