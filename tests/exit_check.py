"""The checker of the exit-mode ray queries and the lensed sky (RRT_TRACE_EXIT,
RRT_SPACETIME_LENSED_SKY), all of it CPU restatement.

Schwarzschild: a numpy restatement of BlackHole::next_micro_ray (blackhole.cpp:17-40, operations in
the reference's order, IEEE double, no contraction), stepped for all rays of a set at once.  It
must reproduce ro_micro_chain's rows bit for bit (tests/test_lensed_sky_rule.py) and is the source
of each row's orbital-plane state (x_axis, y_axis, u, u' before the update, v = u after it), the
escape row j* (the first row whose v is not > 0, NaN included) and the exit direction
    s = sqrt(u u + u' u'),  e = ((-u') / s) x_axis + (u / s) y_axis     (escaped iff u, u' finite, u' < 0)
Kerr: the exit row K of ro_kerr_chain (which has no escape cutoff) is the first row >= steps - 1
whose end point q has |q|^2 > (RRT_SKY_FAR_M M)^2; the exit direction is that row's unit chord.
"""
import math

import numpy as np

import oracle_lib as ol
import rrt
import trace_check as tc

MISS, HIT, CAPTURED, ESCAPED = rrt.RRT_RAY_MISS, rrt.RRT_RAY_HIT, rrt.RRT_RAY_CAPTURED, rrt.RRT_RAY_ESCAPED


def _norm2(v):
    return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]


class Chains:
    """The stepper's rows for rays (o [n, 3], d [n, 3]) under bh = (cx, cy, cz, r_s, dtheta):
    seg [rows, n, 7] = (o3, d3, max_t) of each row's segment, and per row x, y [rows, n, 3], u, up,
    v [rows, n]; jstar [n] (= rows when no row escapes), e [n, 3], escaped [n]."""

    def __init__(self, bh, o, d):
        o = np.ascontiguousarray(o, np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
        n = len(o)
        c = [float(bh[0]), float(bh[1]), float(bh[2])]
        r, dt = float(bh[3]), float(bh[4])
        cos_dt, sin_dt = math.cos(dt), math.sin(dt)  # the host libm's, as blackhole.cpp:36-37
        k = 3.0 * r
        rows = tc.steps_of(dt)
        self.rows, self.n = rows, n
        self.seg = np.zeros((rows, n, 7))
        self.x, self.y = np.zeros((rows, n, 3)), np.zeros((rows, n, 3))
        self.u, self.up, self.v = np.zeros((rows, n)), np.zeros((rows, n)), np.zeros((rows, n))
        ro = [o[:, i].copy() for i in range(3)]
        rd = [d[:, i].copy() for i in range(3)]
        mt = np.zeros(n)
        with np.errstate(all="ignore"):
            for j in range(rows):
                no = [ro[i] + rd[i] * mt for i in range(3)]
                x = [no[i] - c[i] for i in range(3)]
                dist = np.sqrt(_norm2(x))
                ci = 1.0 / dist
                x = [x[i] * ci for i in range(3)]
                u = 1 / dist
                dx = rd[0] * x[0] + rd[1] * x[1] + rd[2] * x[2]
                y = [rd[i] - dx * x[i] for i in range(3)]
                dy = np.sqrt(_norm2(y))
                ci = 1.0 / dy
                y = [y[i] * ci for i in range(3)]
                up = -u * dx / dy
                f1 = -u + k * u * u / 2.0
                u2 = u + up * dt / 2.0
                f2 = -u2 + k * u2 * u2 / 2.0
                u3 = u + up * dt / 2.0 + f1 * dt * dt / 4.0
                f3 = -u3 + k * u3 * u3 / 2.0
                v = u + (up * dt + (f1 + f2 + f3) * dt * dt / 6.0)
                dd = 1 / v
                nx, ny = dd * cos_dt, dd * sin_dt
                nd = [((c[i] + nx * x[i]) + ny * y[i]) - no[i] for i in range(3)]
                mt = np.sqrt(_norm2(nd))
                ci = 1.0 / mt
                rd = [nd[i] * ci for i in range(3)]
                ro = no
                for i in range(3):
                    self.seg[j, :, i], self.seg[j, :, 3 + i] = ro[i], rd[i]
                    self.x[j, :, i], self.y[j, :, i] = x[i], y[i]
                self.seg[j, :, 6] = mt
                self.u[j], self.up[j], self.v[j] = u, up, v
            esc = ~(self.v > 0.0)  # NaN counts
            self.jstar = np.where(esc.any(0), esc.argmax(0), rows)
            jj = np.minimum(self.jstar, rows - 1)
            idx = np.arange(n)
            u, up = self.u[jj, idx], self.up[jj, idx]
            s = np.sqrt(u * u + up * up)
            cx, cy = (-up) / s, u / s
            self.e = cx[:, None] * self.x[jj, idx] + cy[:, None] * self.y[jj, idx]
            self.escaped = (self.jstar < rows) & np.isfinite(u) & np.isfinite(up) & (up < 0.0)


def expected_exit_records(ch, unflagged):
    """The flagged (RRT_TRACE_EXIT) closest-hit records of a Schwarzschild ray set from its checked
    unflagged records and the chains: a record whose row (steps - 1) lies before j* stays; any other
    becomes ESCAPED (MISS where e is undefined) with steps = j* + 1, w_out = -e, the rest 0 / -1."""
    out = unflagged.copy()
    for i in range(len(out)):
        js = int(ch.jstar[i])
        st, steps = int(unflagged[i]["status"]), int(unflagged[i]["steps"])
        if js >= ch.rows or (st in (HIT, CAPTURED) and steps - 1 < js):
            continue
        r = np.zeros((), rrt.HIT_DTYPE)
        r["prim"], r["bsdf"], r["steps"] = -1, -1, js + 1
        if ch.escaped[i]:
            r["status"], r["w_out"] = ESCAPED, -ch.e[i]
        out[i] = r
    return out


def as_any(rec):
    """The shadow query's records of closest-hit records: status, steps and an ESCAPED record's w_out
    stay, every hit field 0 / -1."""
    out = np.zeros(len(rec), rrt.HIT_DTYPE).reshape(rec.shape)
    out["prim"], out["bsdf"] = -1, -1
    out["status"], out["steps"] = rec["status"], rec["steps"]
    esc = rec["status"] == ESCAPED
    out["w_out"][esc] = rec["w_out"][esc]
    return out


def kerr_far2(bh):
    f = rrt.RRT_SKY_FAR_M * (0.5 * bh[3])
    return f * f


def kerr_exit_row(bh, kerr, o, d, steps, budget):
    """(K, -d3 of row K) of the ray's far march, or None when it takes more than `budget` steps: K is
    the first row >= steps - 1 of ro_kerr_chain whose end point lies beyond RRT_SKY_FAR_M M."""
    rows = steps - 1 + budget
    ch, _ = ol.kerr_chain(bh, kerr[0], kerr[1], o, d, max_rows=rows)
    far2 = kerr_far2(bh)
    for K in range(steps - 1, len(ch)):
        q = ch[K, 8:11]
        if (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2] > far2:
            return K, -ch[K, 3:6]
    return None


def kerr_budget_end(bh, kerr, o, d, steps, max_steps):
    """Did the unflagged Kerr march of `steps` steps end on its budget (the swept angle reached 2 pi
    after a step, or the step count ran out) and not in an escape?"""
    _, extra = ol.kerr_chain_st(bh, kerr[0], kerr[1], o, d, 1.0, max_rows=steps)
    return steps >= max_steps or (len(extra) >= steps and extra[steps - 1, 0] >= 2.0 * np.pi)


def angle(a, b):
    """Angle between vectors [n, 3] (atan2 form: accurate for small angles)."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))
