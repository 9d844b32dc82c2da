"""A numpy ray caster for tb_render, written from the rule stated at the top of tennisbot_rl_amd/csrc/tb_render.hpp (camera, five convex
primitives, nearest hit, shading) -- not from the kernel. `render(..., dtype=np.float64)` is the reference, the same code with
dtype=np.float32 its float32 twin. `reference(...)` also marks the AMBIGUOUS pixels of a view, the only ones a comparison may leave out:
  * the float64 id changes when the ray is moved by +-1/16 pixel in x or in y,
  * the two nearest hits (of different primitives) differ by less than 1e-4 max(1, t),
  * the drop shadow's border: a ground pixel whose shadow flag changes under the same four moves.
The fixtures of the render tests (states, views) live here too, so the CPU and the GPU tests share them."""
import math

import numpy as np

from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, F_NET, STATE_ROWS, STATE_WORDS, default_params

BASE = np.array([[135, 190, 235], [60, 140, 80], [235, 235, 235], [220, 60, 50], [230, 240, 40], [40, 60, 200]], np.float64)
ID_SKY, ID_GROUND, ID_NET, ID_GOAL, ID_BALL, ID_RACKET = range(6)
DEFAULT_LIGHT = (0.3, -0.5, 0.8)
JITTER = 1.0 / 16.0
NEAR_TIE = 1e-4
CAP = 0.03


# ------------------------------------------------------------------------------------------------------------ state words
def make_words(kind, envs):
    """[W][N] uint32 from a list of dicts keyed by the names of params.STATE_ROWS (missing rows: 0, quaternion identity, scale 1)"""
    names = STATE_ROWS[kind]
    n = len(envs)
    vals = np.zeros((STATE_WORDS[kind], n), np.float32)
    for e, env in enumerate(envs):
        fields = {k: v for k, v in dict(racket_quat=(0.0, 0.0, 0.0, 1.0), racket_scale=(1.0,), init_dist=(1.0,)).items() if k in names}
        fields.update(env)
        for name, v in fields.items():
            rows = [i for i, nm in enumerate(names) if nm == name]
            assert rows, "unknown state row %r" % name
            vals[rows, e] = np.asarray(v, np.float32).reshape(len(rows))
    words = vals.view(np.uint32).copy()
    words[-2:] = 0  # step count, episode index
    return words


def scene_of(kind, params, words, env):
    """what the renderer reads of env `env`: float64 copies of the float32 values the kernel sees"""
    f = words.view(np.float32).astype(np.float64)[:, env]
    names = STATE_ROWS[kind]

    def rows(name):
        return f[[i for i, nm in enumerate(names) if nm == name]]
    hull = np.ctypeslib.as_array(params.hull_edges)[: params.n_hull].astype(np.float64)
    return dict(kind=kind, ground_half=np.array(list(params.ground_half), np.float64), net_half=np.array(list(params.net_half), np.float64),
                net=bool(params.flags & F_NET), goal=rows("goal") if kind == ENV_SWING else None, goal_radius=float(params.goal_radius),
                goal_half_len=float(params.goal_half_len), ball=rows("ball_pos"), ball_radius=float(params.ball_radius), com=rows("racket_pos"),
                quat=rows("racket_quat"), scale=float(rows("racket_scale")[0]) if kind == ENV_TENNIS else float(params.racket_scale),
                half_thick=float(params.racket_half_thick), hull_a=hull[:, 0:2], hull_e=hull[:, 2:4])


# ------------------------------------------------------------------------------------------------------------ camera
def camera_basis(eye, target, up, fov_y_deg, W, H):
    """f, th (W / H) r, th u in float64, then rounded to float32 as the library hands them to the kernel"""
    eye, target, up = (np.asarray(x, np.float32).astype(np.float64) for x in (eye, target, up))
    f = target - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    th = math.tan(0.5 * float(np.float32(fov_y_deg)) * math.pi / 180.0)
    r32 = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    return dict(f=r32(f), r=r32(th * W / H * r), u=r32(th * u), unit=(f, r, u), th=th)


def unit_light(light=DEFAULT_LIGHT):
    l = np.asarray(light, np.float32).astype(np.float64)
    return (l / np.linalg.norm(l)).astype(np.float32).astype(np.float64)


def ray_directions(basis, W, H, dtype, dx=0.0, dy=0.0):
    """[H, W, 3] unit directions through the pixel centres moved by (dx, dy) pixels"""
    i = np.arange(W, dtype=np.float64)[None, :] + dx
    j = np.arange(H, dtype=np.float64)[:, None] + dy
    sx = ((2.0 * i + 1.0 - W) / W).astype(dtype)
    sy = ((H - 2.0 * j - 1.0) / H).astype(dtype)
    if dx == 0.0 and dy == 0.0:  # the kernel's own form: exact integer numerators, one division
        sx = ((2 * np.arange(W)[None, :] + 1 - W).astype(dtype) / dtype(W))
        sy = ((H - 2 * np.arange(H)[:, None] - 1).astype(dtype) / dtype(H))
    f, r, u = (basis[k].astype(dtype) for k in ("f", "r", "u"))
    d = f[None, None, :] + sx[..., None] * r[None, None, :] + sy[..., None] * u[None, None, :]
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


# ------------------------------------------------------------------------------------------------------------ convex spans
class Span:
    """the ray is inside a convex solid for t in [t0, t1]; n0 / n1 the outward normals of the constraints that gave them"""

    def __init__(self, shape, dtype):
        self.t0 = np.full(shape, -np.inf, dtype)
        self.t1 = np.full(shape, np.inf, dtype)
        self.n0 = np.zeros(shape + (3,), dtype)
        self.n1 = np.zeros(shape + (3,), dtype)
        self.ok = np.ones(shape, bool)

    def clip(self, t, applies, enters, n):
        m = applies & enters & (t > self.t0)
        self.t0 = np.where(m, t, self.t0)
        self.n0 = np.where(m[..., None], n, self.n0)
        m = applies & ~enters & (t < self.t1)
        self.t1 = np.where(m, t, self.t1)
        self.n1 = np.where(m[..., None], n, self.n1)

    def slab(self, o, d, h, axis):
        """|o + t d| <= h along `axis` (a unit vector); o a scalar or an array, d an array"""
        dtype = d.dtype.type
        o = np.broadcast_to(np.asarray(o, dtype), d.shape)
        nz = d != 0
        with np.errstate(all="ignore"):
            inv = dtype(1) / np.where(nz, d, dtype(1))
            pos = d > 0
            axis = np.asarray(axis, dtype)
            frm = np.where(pos[..., None], -axis, axis)
            h = dtype(h)
            self.clip((np.where(pos, -h, h) - o) * inv, nz, np.ones_like(nz), frm)
            self.clip((np.where(pos, h, -h) - o) * inv, nz, np.zeros_like(nz), -frm)
            self.ok &= nz | (np.abs(o) <= h)

    def round(self, oc, d, R, flat):
        """ball (flat: disc in x, y) of radius R around the origin of oc, closest-approach form"""
        dtype = d.dtype.type
        oc = np.broadcast_to(np.asarray(oc, dtype), d.shape).copy()
        d = d.copy()
        if flat:
            oc[..., 2] = 0
            d[..., 2] = 0
        R = dtype(R)
        with np.errstate(all="ignore"):
            a = (d * d).sum(-1)
            nz = a != 0
            a1 = np.where(nz, a, dtype(1))
            tm = -(oc * d).sum(-1) / a1
            p = oc + tm[..., None] * d
            h2 = (R * R - (p * p).sum(-1)) / a1
            good = nz & (h2 >= 0)
            h = np.sqrt(np.where(good, h2, dtype(0)))
            self.clip(tm - h, good, np.ones_like(nz), p - h[..., None] * d)
            self.clip(tm + h, good, np.zeros_like(nz), p + h[..., None] * d)
            self.ok &= np.where(nz, h2 >= 0, (oc * oc).sum(-1) <= R * R)

    def hit(self):
        """(t, facing normal, hit?) of the solid: the entry when t0 >= 0, else the exit"""
        with np.errstate(all="ignore"):
            entry = self.t0 >= 0
            t = np.where(entry, self.t0, self.t1)
            n = np.where(entry[..., None], self.n0, -self.n1)
            return t, n, self.ok & (self.t0 <= self.t1) & (t >= 0) & (t < np.inf)


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def box_span(o, d, half):
    sp = Span(d.shape[:-1], d.dtype.type)
    for k in range(3):
        sp.slab(o[k], d[..., k], half[k], np.eye(3)[k])
    return sp


def racket_span(sc, o, d):
    dtype = d.dtype.type
    R = quat_matrix(sc["quat"].astype(dtype)).astype(dtype)
    s = dtype(sc["scale"])
    ob = R.T @ (o - sc["com"].astype(dtype))
    db = d @ R  # rows: R^T d
    sp = Span(d.shape[:-1], dtype)
    sp.slab(ob[0], db[..., 0], dtype(sc["half_thick"]) * s, (1.0, 0.0, 0.0))
    for a, e in zip(sc["hull_a"].astype(dtype), sc["hull_e"].astype(dtype)):
        ny, nz = e[1], -e[0]
        num = ny * (ob[1] - a[0] * s) + nz * (ob[2] - a[1] * s)
        den = ny * db[..., 1] + nz * db[..., 2]
        nzr = den != 0
        with np.errstate(all="ignore"):
            t = -num / np.where(nzr, den, dtype(1))
        n = np.broadcast_to(np.array([0, ny, nz], dtype), d.shape)
        sp.clip(t, nzr, den < 0, n)
        sp.ok &= nzr | (num <= 0)
    sp.n0 = sp.n0 @ R.T  # back to the world
    sp.n1 = sp.n1 @ R.T
    return sp


def cast(sc, o, d):
    """every primitive's hit along the rays (o, d [.., 3]): per-primitive t [5, ..] (+inf: no hit), the nearest's id, t and normal"""
    dtype = d.dtype.type
    o = np.asarray(o, dtype)
    shape = d.shape[:-1]
    ts = np.full((5,) + shape, np.inf, dtype)
    ns = np.zeros((5,) + shape + (3,), dtype)

    def put(k, sp):
        t, n, ok = sp.hit()
        ts[k] = np.where(ok, t, np.inf)
        ns[k] = n
    if np.all(np.isfinite(o)):
        put(0, box_span(o, d, sc["ground_half"]))
        if sc["net"]:
            put(1, box_span(o, d, sc["net_half"]))
        if sc["goal"] is not None and np.all(np.isfinite(sc["goal"])):
            g = sc["goal"].astype(dtype)
            sp = Span(shape, dtype)
            sp.round(np.array([o[0] - g[0], o[1] - g[1], 0], dtype), d, sc["goal_radius"], True)
            sp.slab(o[2], d[..., 2], sc["goal_half_len"], (0.0, 0.0, 1.0))
            put(2, sp)
        if np.all(np.isfinite(sc["ball"])):
            sp = Span(shape, dtype)
            sp.round(o - sc["ball"].astype(dtype), d, sc["ball_radius"], False)
            put(3, sp)
        if np.all(np.isfinite(sc["com"])) and np.all(np.isfinite(sc["quat"])) and np.isfinite(sc["scale"]) and sc["scale"] > 0:
            put(4, racket_span(sc, o, d))
    ids = np.zeros(shape, np.int64)
    best = np.full(shape, np.inf, dtype)
    normal = np.zeros(shape + (3,), dtype)
    for k in range(5):  # a later primitive only where strictly nearer
        m = ts[k] < best
        best = np.where(m, ts[k], best)
        ids = np.where(m, k + 1, ids)
        normal = np.where(m[..., None], ns[k], normal)
    return ts, ids, best, normal


def shadowed(sc, o, d, ids, t):
    dtype = d.dtype.type
    ball = sc["ball"].astype(dtype)
    if not (np.all(np.isfinite(ball)) and ball[2] > dtype(sc["ground_half"][2])):
        return np.zeros(ids.shape, bool)
    with np.errstate(all="ignore"):
        tt = np.where(ids == ID_GROUND, t, dtype(0))
        hx = o[0] + tt * d[..., 0] - ball[0]
        hy = o[1] + tt * d[..., 1] - ball[1]
        rr = dtype(2) * dtype(sc["ball_radius"])
        return (ids == ID_GROUND) & (hx * hx + hy * hy < rr * rr)


def render(sc, eye, basis, W, H, dtype=np.float64, light=None, dx=0.0, dy=0.0):
    """ids [H, W], depth [H, W] (+inf sky), rgb uint8 [H, W, 3], shadow flags, per-primitive hits"""
    o = np.asarray(eye, np.float32).astype(dtype)
    d = ray_directions(basis, W, H, dtype, dx, dy)
    ts, ids, t, n = cast(sc, o, d)
    l = (unit_light() if light is None else unit_light(light)).astype(dtype)
    with np.errstate(all="ignore"):
        nn = n / np.sqrt(np.where(ids[..., None] > 0, (n * n).sum(-1, keepdims=True), dtype(1)))
        ndl = np.clip((nn * l).sum(-1), dtype(0), dtype(1))
    shade = np.where(ids > 0, dtype(0.35) + dtype(0.65) * ndl, dtype(1))
    sh = shadowed(sc, o, d, ids, t)
    shade = np.where(sh, shade * dtype(0.5), shade)
    colour = BASE.astype(dtype)[ids] * shade[..., None]
    rgb = np.floor(colour + dtype(0.5)).astype(np.uint8)
    return dict(ids=ids.astype(np.uint8), depth=t, rgb=rgb, shadow=sh, hits=ts, colour=colour)


def reference(sc, eye, basis, W, H, light=None):
    """the float64 render, its float32 twin and the ambiguous mask of one view"""
    r64 = render(sc, eye, basis, W, H, np.float64, light)
    r32 = render(sc, eye, basis, W, H, np.float32, light)
    amb = np.zeros((H, W), bool)
    for dx, dy in ((JITTER, 0.0), (-JITTER, 0.0), (0.0, JITTER), (0.0, -JITTER)):
        rj = render(sc, eye, basis, W, H, np.float64, light, dx, dy)
        amb |= (rj["ids"] != r64["ids"]) | (rj["shadow"] != r64["shadow"])
    hs = np.sort(r64["hits"], axis=0)
    with np.errstate(all="ignore"):
        amb |= np.isfinite(hs[1]) & (hs[1] - hs[0] < NEAR_TIE * np.maximum(1.0, hs[0]))
    return dict(f64=r64, f32=r32, ambiguous=amb, share=float(amb.mean()))


# ------------------------------------------------------------------------------------------------------------ fixtures
_Q_SWING = (0.0, math.sin(0.25), 0.0, math.cos(0.25))
_Q_TENNIS = tuple(np.array([0.1, 0.2, 0.05, 0.97]) / np.linalg.norm([0.1, 0.2, 0.05, 0.97]))
SWING_ENVS = [dict(racket_pos=(3.0, 0.1, 0.84), racket_quat=_Q_SWING, ball_pos=(2.9, 0.1, 1.3), goal=(-12.0, 1.0)),
              dict(racket_pos=(3.0, 0.1, 0.84), racket_quat=_Q_SWING, ball_pos=(2.96, 0.12, 0.95), goal=(-12.0, 1.0))]
TENNIS_ENVS = [dict(racket_pos=(9.5, 0.3, 0.55), racket_quat=_Q_TENNIS, ball_pos=(4.0, 0.6, 1.4), racket_scale=(3.0,)),
               dict(racket_pos=(9.5, 0.3, 0.55), racket_quat=_Q_TENNIS, ball_pos=(4.0, 0.6, 1.4), racket_scale=(1.0,))]
ENVS = {ENV_SWING: SWING_ENVS, ENV_TENNIS: TENNIS_ENVS}

# name, env kind, env of the block above, eye, target, fov
VIEWS = [
    ("swing_court", ENV_SWING, 0, (9, -7, 5), (-3, 0, .5), 60.0),
    ("swing_near", ENV_SWING, 0, (3.9, -.5, 1.35), (2.95, .1, 1.05), 60.0),
    ("swing_ball_at_racket", ENV_SWING, 1, (3.7, -.3, 1.2), (2.97, .1, .9), 60.0),
    ("tennis_court", ENV_TENNIS, 0, (16, -8, 6), (2, 0, .5), 60.0),
    ("tennis_along", ENV_TENNIS, 0, (13, .3, 2), (0, 0, 1), 60.0),
    ("tennis_near", ENV_TENNIS, 0, (11.5, -1.2, 1.6), (9, .4, 1), 60.0),
    ("tennis_near_scale1", ENV_TENNIS, 1, (11.5, -1.2, 1.6), (9, .4, 1), 60.0),
    # 0.35 m from the ball (3.35 cm): fov 40 puts it on > 100 pixels of 64 x 48
    ("swing_ball_closeup", ENV_SWING, 0, (3.15, -0.14, 1.35), (2.9, 0.1, 1.3), 40.0),
    # down onto the court under the ball: the drop shadow (none of the views above shows it)
    ("swing_shadow", ENV_SWING, 0, (3.3, -0.3, 0.6), (2.9, 0.1, 0.0), 40.0),
    # a horizontal view direction: with an odd H the centre row has d_z == 0 exactly -- parallel to every z slab, inside the net's
    ("tennis_horizontal", ENV_TENNIS, 0, (12.0, -2.0, 0.25), (9.0, 0.5, 0.25), 60.0),
]
VIEW_NAMES = [v[0] for v in VIEWS]
SIZES = [(64, 48), (17, 9)]
UP = (0.0, 0.0, 1.0)
_CACHE = {}


def fixture_params():
    return default_params()


def fixture_words(kind):
    return make_words(kind, ENVS[kind])


def fixture(name, W, H):
    """the reference of one view at one size: computed once, shared by every test that asks, never changed"""
    key = (name, W, H)
    if key not in _CACHE:
        _, kind, env, eye, target, fov = VIEWS[VIEW_NAMES.index(name)]
        params = fixture_params()
        sc = scene_of(kind, params, fixture_words(kind), env)
        ref = reference(sc, eye, camera_basis(eye, target, UP, fov, W, H), W, H)
        ref.update(kind=kind, env=env, eye=eye, target=target, fov=fov, scene=sc)
        for k in ("ids", "depth", "rgb", "shadow", "hits", "colour"):
            ref["f64"][k].setflags(write=False)
            ref["f32"][k].setflags(write=False)
        ref["ambiguous"].setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]
