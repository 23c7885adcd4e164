"""The CPU rule of the moving observer (rrt_set_observer), restated from DESIGN.md §16 in
IEEE double with the operations in the order fixed there: the host constants one Python float operation
at a time (rrt_host.cpp resolve_observer), the per-ray rule in numpy float64 element by element
(rrt_device.h observer_ray; numpy's + - x / sqrt are correctly rounded and nothing is contracted).

It reuses disk_check.Hole (M, a, the local frame) and restates kerr_fl at the camera.  Beyond the rule
it gives what the physics pins of tests/test_observer_rule.py need: the Kerr-Schild metric at the
camera, the static observer's tetrad and the camera's four-velocity.
"""
import math

import numpy as np

import disk_check as dc

STATIC, COORDINATE = "static", "coordinate"


def kerr_fl(hole, pos):
    """rrt_device.h kerr_fl at world point pos: (f, l local [3], r)."""
    h = hole
    q = h.local([float(pos[i]) - h.c[i] for i in range(3)])
    zz = q[2] * q[2]
    w = ((q[0] * q[0] + q[1] * q[1]) + zz) - h.a2
    r2 = 0.5 * w + math.sqrt(0.25 * (w * w) + h.a2 * zz)
    r = math.sqrt(r2)
    iw = 1.0 / (r2 + h.a2)
    l = [(r * q[0] + h.a * q[1]) * iw, (r * q[1] - h.a * q[0]) * iw, q[2] / r]
    f = ((2.0 * h.m) * (r * r2)) / (r2 * r2 + h.a2 * zz)
    return f, l, r


class Observer:
    """The launch constants of an observer (rrt_internal.h DObs) for a camera position and a hole:
    f, sg, alpha, dg, ig, gamma, kappa, lw [3], b2, identity; beta [3]."""

    def __init__(self, hole, cam_pos, velocity, frame=STATIC):
        self.hole, self.frame = hole, frame
        self.f, l, self.r = kerr_fl(hole, cam_pos)
        self.l_local = l
        self.lw = [(hole.ex[i] * l[0] + hole.ey[i] * l[1]) + hole.ez[i] * l[2] for i in range(3)]
        coord = frame == COORDINATE
        self.sg = math.sqrt(1.0 - self.f) if self.f <= 1.0 else math.nan
        self.alpha = 0.0 if coord else self.sg - 1.0
        self.dg = 1.0 if coord else 1.0 / self.sg
        b = [float(v) for v in velocity]
        self.beta = b
        self.b2 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
        self.ig = math.sqrt(1.0 - self.b2)
        self.gamma = 1.0 / self.ig
        self.kappa = self.gamma / (self.gamma + 1.0)
        self.identity = coord and b[0] == 0.0 and b[1] == 0.0 and b[2] == 0.0

    def resolved(self):
        """rrt_get_observer's resolved[12]."""
        return np.array([self.f, self.sg, self.alpha, self.dg, self.ig, self.gamma, self.kappa, self.lw[0], self.lw[1],
                         self.lw[2], self.b2, 1.0 if self.identity else 0.0])


def static_direction(ob, npr):
    """n [m, 3], iden [m]: the static-frame viewing direction of the rest-frame directions npr [m, 3]."""
    npr = np.asarray(npr, np.float64).reshape(-1, 3)
    b = ob.beta
    s = (b[0] * npr[:, 0] + b[1] * npr[:, 1]) + b[2] * npr[:, 2]
    c = 1.0 - ob.kappa * s
    iden = 1.0 / (1.0 - s)
    n = np.stack([(npr[:, i] * ob.ig - b[i] * c) * iden for i in range(3)], axis=1)
    return n, iden


def observer_ray(ob, npr):
    """rrt_device.h observer_ray on npr [m, 3]: (d_eff [m, 3], D_v [m], D [m]).  The identity observer
    passes the directions through with both ratios 1, as the kernels do."""
    npr = np.asarray(npr, np.float64).reshape(-1, 3)
    if ob.identity:
        return npr.copy(), np.ones(len(npr)), np.ones(len(npr))
    n, iden = static_direction(ob, npr)
    lw = ob.lw
    t = (lw[0] * n[:, 0] + lw[1] * n[:, 1]) + lw[2] * n[:, 2]
    at = ob.alpha * t
    k = np.stack([n[:, i] + at * lw[i] for i in range(3)], axis=1)
    r = 1.0 / np.sqrt((k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1]) + k[:, 2] * k[:, 2])  # rrt_device.h unit
    d_eff = np.stack([r * k[:, i] for i in range(3)], axis=1)
    dv = ob.ig * iden
    return d_eff, dv, ob.dg * dv


def weight(x):
    """The beaming weight of an energy ratio: (float)((x x) (x x))."""
    x = np.asarray(x, np.float64)
    x2 = x * x
    return (x2 * x2).astype(np.float32)


# ------------------------------------------------------------------ the physics behind the rule
def metric(ob):
    """g_mn = eta + f l (x) l at the camera, in (t, world x, y, z); l_m = (1, l_w)."""
    lm = np.array([1.0] + list(ob.lw))
    return np.diag([-1.0, 1.0, 1.0, 1.0]) + ob.f * np.outer(lm, lm)


def tetrad(ob):
    """(u_s [4], e [3, 4]): the static observer's four-velocity and the symmetric orthonormalisation
    of the world axes, e(v) = (f (l.v) / sg ; v + alpha (l.v) l)."""
    lw = np.array(ob.lw)
    sg = math.sqrt(1.0 - ob.f)
    al = sg - 1.0
    u = np.array([1.0 / sg, 0.0, 0.0, 0.0])
    e = np.zeros((3, 4))
    for i in range(3):
        v = np.zeros(3)
        v[i] = 1.0
        lv = float(lw @ v)
        e[i, 0] = ob.f * lv / sg
        e[i, 1:] = v + al * lv * lw
    return u, e


def camera_velocity(ob):
    """u_cam = gamma (u_s + beta^i e_i)."""
    u, e = tetrad(ob)
    return ob.gamma * (u + np.array(ob.beta) @ e)


# ------------------------------------------------------------------ what the tests use
def gpu_velocity(cam_c2w):
    """The GPU tests' velocity: 0.4 c0 + 0.1 c1 - 0.2 c2, c0..c2 the columns of the camera's c2w
    (row-major [9])."""
    m = np.asarray(cam_c2w, np.float64).reshape(3, 3)
    return 0.4 * m[:, 0] + 0.1 * m[:, 1] - 0.2 * m[:, 2]


def moved_position(hole, pos, r_m):
    """The point r_m M from the hole on the line from the hole through pos."""
    c = np.array(hole.c)
    v = np.asarray(pos, np.float64) - c
    return c + v * (r_m * hole.m / np.linalg.norm(v))


def observer_camera(hole=None, r_m=None):
    """The camera of the observer frames: the wide golden camera's pose (cfg1_spheres_480x360_s8) with a
    50 x 38.5 degree field of view -- wide enough for D_v to span both sides of 1 under gpu_velocity -- as an
    rrt.CameraDesc; with hole and r_m, moved to r_m M from the hole."""
    import rrt
    from golden_cases import Case
    cam = rrt.load_camera(Case("cfg1_spheres_480x360_s8").camera_path)
    cam.hFov, cam.vFov = 50.0, 38.5
    if r_m is not None:
        p = moved_position(hole, list(cam.pos), r_m)
        cam.pos[0], cam.pos[1], cam.pos[2] = p
    return cam


def pixel_directions(cam, w, h, stride=1):
    """The pixel-centre directions of an rrt.CameraDesc on a w x h frame (every stride-th pixel both
    ways), row-major, y = 0 at the bottom: Camera::generate_ray by the restatement (ro_camera_ray)."""
    import ctypes as C

    import oracle_lib as ol
    cols = np.array(list(cam.c2w), np.float64).reshape(3, 3).T.ravel().copy()
    pos = np.array(list(cam.pos), np.float64)
    xs, ys = (a.ravel() for a in np.meshgrid(np.arange(0, w, stride), np.arange(0, h, stride)))
    o, d = np.zeros((len(xs), 3)), np.zeros((len(xs), 3))
    mn, mx = C.c_double(), C.c_double()
    for i, (x, y) in enumerate(zip(xs, ys)):
        ol.lib().ro_camera_ray(cam.hFov, cam.vFov, pos, cols, cam.nClip, cam.fClip, (x + 0.5) / w, (y + 0.5) / h, o[i], d[i],
                               C.byref(mn), C.byref(mx))
    return d
