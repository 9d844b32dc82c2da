"""Labelled forced states for the ball's static contacts -- court, net, goal -- region by region of the static narrowphase
(sphere_vs_box's faces, edges, corners and interior; sphere_vs_goal's cap, wall, rim, interior and axis), with several static rows in
one solve and a racket row on top of them. tests/test_static_contact_states.py pins what the batch reaches on the oracle alone,
tests/test_gpu_static_contacts.py holds the kernels to the oracle on it.

LANES = 64 lanes per region. Lane slot s of a region draws the ball's surface distance d to the region's shape by s % 3:
deep (-4 mm .. 0), shallow (0 .. contact_threshold), graze (contact_threshold x [0.97, 1.03]: hit and no-hit both occur); the ball's
velocity points towards the shape at 0 .. 25 m/s except where s % 8 == 7 (it separates). The direction from the nearest feature is
uniform over that feature's normal cone; an edge's angle is drawn from (0.051, pi/2 - 0.051), inside the (0.05, pi/2 - 0.05) that
keeps both components of the normal above 0.05 (sin 0.05 = 0.04998).

Two lane orders: "blocked" (region k in lanes 64 k .. 64 k + 63: whole waves are uniform) and "interleaved" (lane i holds region i mod R:
every wave mixes all regions) -- the same states permuted -- each followed by the same 37 extra lanes of mixed regions, so that n is no
multiple of 64."""
import numpy as np

from helpers import make_words
from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, default_params

SEED = 4242
LANES = 64
EXTRA = 37
ROW_RACKET, ROW_GROUND, ROW_NET, ROW_GOAL = 1, 2, 4, 8   # the kernels' CT_* bits: 1 << row
DEEP, SHALLOW, GRAZE = 0, 1, 2

_COMMON = ["high", "g_top", "g_edge_x", "g_edge_y", "g_corner", "g_side", "g_under", "n_face", "n_top", "n_tape", "n_end", "n_end_edge",
           "n_corner", "n_inside", "n_foot"]
REGIONS = {ENV_TENNIS: _COMMON + ["r_foot"],
           ENV_SWING: _COMMON + ["c_top", "c_wall", "c_rim", "c_inside", "c_axis", "c_net", "r_foot"]}
EDGE_REGIONS = ("g_edge_x", "g_edge_y", "g_corner", "n_tape", "n_end_edge", "n_corner", "c_rim")   # oblique normals
RACKET_PARK = {ENV_TENNIS: (10.0, 0.0, 1.0), ENV_SWING: (9.0, 0.0, 1.0)}


def _rot(q, v):
    u, w = q[:, :3], q[:, 3:4]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


class _Draw:
    """the draws of one list of (region, slot) lanes"""

    def __init__(self, kind, rng):
        self.kind, self.rng, self.p = kind, rng, default_params()
        p = self.p
        self.r, self.thr = float(p.ball_radius), float(p.contact_threshold)
        self.gh = [float(x) for x in p.ground_half]
        self.nh = [float(x) for x in p.net_half]
        self.R, self.hl = float(p.goal_radius), float(p.goal_half_len)
        self.xmax = 13.9 if kind == ENV_SWING else 10.3   # Tennisbot's episode ends where the ball is 0.5 m past the parked racket

    def dist(self, slot):
        """surface distance by the slot's third"""
        rng, thr, third = self.rng, self.thr, slot % 3
        n = len(slot)
        d = np.where(third == DEEP, rng.uniform(-0.004, -0.02 * thr, n),
                     np.where(third == SHALLOW, rng.uniform(0.02 * thr, 0.98 * thr, n), thr * rng.uniform(0.97, 1.03, n)))
        return d

    def solid(self, slot):
        """a distance that always hits (the second shape of a two-row region)"""
        return np.where(slot % 2 == 0, self.rng.uniform(-0.003, -0.02 * self.thr, len(slot)), self.rng.uniform(0.02 * self.thr, 0.9 * self.thr, len(slot)))

    def sign(self, n):
        return np.where(self.rng.random(n) < 0.5, -1.0, 1.0)

    def angle(self, n):
        return self.rng.uniform(0.051, 0.5 * np.pi - 0.051, n)

    def octant(self, n):
        """a direction uniform over the positive octant, every component above 0.06"""
        u = np.abs(self.rng.normal(size=(n, 3)))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        while True:
            bad = (u < 0.06).any(1)
            if not bad.any():
                return u
            v = np.abs(self.rng.normal(size=(int(bad.sum()), 3)))
            u[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)

    def court_xy(self, n, ymax=6.9):
        """a spot on the court clear of the net and of where SwingRacket's goals stand (x < -2.4)"""
        x = self.rng.uniform(0.3, self.xmax, n)
        x = np.where((self.rng.random(n) < 0.5) & (x < 2.3), -x, x)
        return x, self.rng.uniform(-ymax, ymax, n)

    def far_goal(self, n):
        return np.stack([self.rng.uniform(-11, -4, n), self.rng.uniform(-4, 4, n)], 1)

    # ------------------------------------------------------------------ the regions: each returns dict(bp, u, rows, primary, sub[, goal, racket...])
    def region(self, name, slot):
        rng, r, thr, n = self.rng, self.r, self.thr, len(slot)
        gh, nh, R, hl = self.gh, self.nh, self.R, self.hl
        z3 = np.zeros(n)
        out = dict(sub=np.zeros(n, np.int64), third=slot % 3)
        d = self.dist(slot)
        rd = r + d
        if name == "high":   # the low point (z - r - thr) above static_top + 1e-3 (static_top: the net's top) by 1 mm .. 1 m
            z = (nh[2] + 1.0e-3) + r + thr + rng.uniform(1.0e-3, 1.0, n)
            out.update(bp=np.stack([rng.uniform(-13.0, 7.0, n), rng.uniform(-6.9, 6.9, n), z], 1), rows=np.zeros(n, np.int64), primary=np.zeros(n, np.int64),
                       u=np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-0.2, 0.2, n)], 1), third=np.full(n, -1), speed=rng.uniform(0, 6, n))
            return out
        if name == "g_top":
            x, y = self.court_xy(n)
            q, u, rows = np.stack([x, y, np.full(n, gh[2])], 1), np.stack([z3, z3, z3 + 1], 1), ROW_GROUND
        elif name == "g_edge_x":   # nout == 2: x and z outside
            sx, a = self.sign(n) if self.kind == ENV_SWING else -np.ones(n), self.angle(n)
            q, u, rows = np.stack([sx * gh[0], rng.uniform(-6.9, 6.9, n), np.full(n, gh[2])], 1), np.stack([sx * np.cos(a), z3, np.sin(a)], 1), ROW_GROUND
        elif name == "g_edge_y":   # y and z outside
            sy, a = self.sign(n), self.angle(n)
            x = rng.uniform(-13.9, self.xmax, n)
            q, u, rows = np.stack([x, sy * gh[1], np.full(n, gh[2])], 1), np.stack([z3, sy * np.cos(a), np.sin(a)], 1), ROW_GROUND
        elif name == "g_corner":   # nout == 3
            sx, sy, o = self.sign(n) if self.kind == ENV_SWING else -np.ones(n), self.sign(n), self.octant(n)
            q, u, rows = np.stack([sx * gh[0], sy * gh[1], np.full(n, gh[2])], 1), o * np.stack([sx, sy, z3 + 1], 1), ROW_GROUND
        elif name == "g_side":     # nout == 1 on x (sub 0) or on y (sub 1), the centre at |z| <= half thickness
            sub = (slot // 3) % 2
            s = self.sign(n)
            if self.kind != ENV_SWING:
                s = np.where(sub == 0, -1.0, s)
            z = rng.uniform(-gh[2], gh[2], n)
            qx = np.stack([s * gh[0], rng.uniform(-6.9, 6.9, n), z], 1)
            qy = np.stack([rng.uniform(-13.9, self.xmax, n), s * gh[1], z], 1)
            q = np.where(sub[:, None] == 0, qx, qy)
            u = np.where(sub[:, None] == 0, np.stack([s, z3, z3], 1), np.stack([z3, s, z3], 1))
            out["sub"], rows = sub, ROW_GROUND
        elif name == "g_under":
            x, y = self.court_xy(n)
            q, u, rows = np.stack([x, y, np.full(n, -gh[2])], 1), np.stack([z3, z3, z3 - 1], 1), ROW_GROUND
        elif name == "n_face":
            sx = self.sign(n)
            q, u, rows = np.stack([sx * nh[0], rng.uniform(-6.2, 6.2, n), rng.uniform(0.06, 0.47, n)], 1), np.stack([sx, z3, z3], 1), ROW_NET
        elif name == "n_top":
            q, u, rows = np.stack([rng.uniform(-0.09, 0.09, n), rng.uniform(-6.2, 6.2, n), np.full(n, nh[2])], 1), np.stack([z3, z3, z3 + 1], 1), ROW_NET
        elif name == "n_tape":     # the top edges along y
            sx, a = self.sign(n), self.angle(n)
            q, u, rows = np.stack([sx * nh[0], rng.uniform(-6.2, 6.2, n), np.full(n, nh[2])], 1), np.stack([sx * np.cos(a), z3, np.sin(a)], 1), ROW_NET
        elif name == "n_end":
            sy = self.sign(n)
            q, u, rows = np.stack([rng.uniform(-0.09, 0.09, n), sy * nh[1], rng.uniform(0.06, 0.47, n)], 1), np.stack([z3, sy, z3], 1), ROW_NET
        elif name == "n_end_edge":  # the (x, y) edges (sub 0) and the (y, z) edges (sub 1)
            sub = (slot // 3) % 2
            sx, sy, a = self.sign(n), self.sign(n), self.angle(n)
            qa, ua = np.stack([sx * nh[0], sy * nh[1], rng.uniform(0.06, 0.47, n)], 1), np.stack([sx * np.cos(a), sy * np.sin(a), z3], 1)
            qb, ub = np.stack([rng.uniform(-0.09, 0.09, n), sy * nh[1], np.full(n, nh[2])], 1), np.stack([z3, sy * np.cos(a), np.sin(a)], 1)
            q, u = np.where(sub[:, None] == 0, qa, qb), np.where(sub[:, None] == 0, ua, ub)
            out["sub"], rows = sub, ROW_NET
        elif name == "n_corner":
            sx, sy, o = self.sign(n), self.sign(n), self.octant(n)
            q, u, rows = np.stack([sx * nh[0], sy * nh[1], np.full(n, nh[2])], 1), o * np.stack([sx, sy, z3 + 1], 1), ROW_NET
        elif name == "n_inside":
            return self.n_inside(slot, out)
        elif name in ("n_foot", "c_net", "r_foot"):   # on the court and against a net face
            sx = self.sign(n)
            dg = self.solid(slot)
            bp = np.stack([sx * (nh[0] + rd), rng.uniform(-6.2, 6.2, n), gh[2] + r + dg], 1)
            u = np.stack([sx, z3, z3 + 1], 1) / np.sqrt(2.0)
            out.update(bp=bp, u=u, rows=np.full(n, ROW_GROUND | ROW_NET), primary=np.full(n, ROW_NET))
            if name == "c_net":   # ... inside a goal centred within 0.6 m: the ball's centre in the cylinder, the cap's face the nearest
                rho, ang = rng.uniform(0.0, 0.6, n), rng.uniform(0, 2 * np.pi, n)
                out["goal"] = bp[:, :2] + np.stack([rho * np.cos(ang), rho * np.sin(ang)], 1)
                out["rows"] = out["rows"] | ROW_GOAL
            if name == "r_foot":
                self.racket_around(out)
            return out
        elif name == "c_top":
            g = self.far_goal(n)
            ang, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 1.45, n)
            q = np.stack([g[:, 0] + rad * np.cos(ang), g[:, 1] + rad * np.sin(ang), np.full(n, hl)], 1)
            u, rows, out["goal"] = np.stack([z3, z3, z3 + 1], 1), ROW_GOAL, g
        elif name == "c_wall":     # on the court and against the wall (sub 0: two rows), against the wall at z in (0.05, 0.12) (sub 1)
            sub = np.isin(slot, (0, 1, 2, 5, 8, 11, 14, 17)).astype(np.int64)   # (mostly graze lanes: the on-court lanes keep 48 with two rows)
            g = self.far_goal(n)
            ang = rng.uniform(0, 2 * np.pi, n)
            rad2 = np.stack([np.cos(ang), np.sin(ang)], 1)
            z = np.where(sub == 0, gh[2] + r + self.solid(slot), rng.uniform(0.05, 0.12, n))
            bp = np.concatenate([g + (R + rd)[:, None] * rad2, z[:, None]], 1)
            u = np.where(sub[:, None] == 0, np.concatenate([rad2, np.ones((n, 1))], 1) / np.sqrt(2.0), np.concatenate([rad2, np.zeros((n, 1))], 1))
            out.update(bp=bp, u=u, rows=np.where(sub == 0, ROW_GROUND | ROW_GOAL, ROW_GOAL), primary=np.full(n, ROW_GOAL), sub=sub, goal=g)
            return out
        elif name == "c_rim":
            g = self.far_goal(n)
            ang, a = rng.uniform(0, 2 * np.pi, n), self.angle(n)
            rad2 = np.stack([np.cos(ang), np.sin(ang)], 1)
            q = np.concatenate([g + R * rad2, np.full((n, 1), hl)], 1)
            u, rows, out["goal"] = np.concatenate([rad2 * np.cos(a)[:, None], np.sin(a)[:, None]], 1), ROW_GOAL, g
        elif name == "c_inside":   # the centre inside the cylinder: nearer the cap (sub 0), nearer the wall (sub 1)
            sub = (slot // 3) % 2
            g = self.far_goal(n)
            ang = rng.uniform(0, 2 * np.pi, n)
            rad2 = np.stack([np.cos(ang), np.sin(ang)], 1)
            rad = np.where(sub == 0, rng.uniform(0.0, 1.4, n), R - rng.uniform(0.001, 0.03, n))
            z = np.where(sub == 0, hl - rng.uniform(0.001, 0.05, n), rng.uniform(0.045, 0.09, n))
            bp = np.concatenate([g + rad[:, None] * rad2, z[:, None]], 1)
            u = np.where(sub[:, None] == 0, np.stack([z3, z3, z3 + 1], 1), np.concatenate([rad2, np.zeros((n, 1))], 1))
            out.update(bp=bp, u=u, rows=np.full(n, ROW_GOAL), primary=np.full(n, ROW_GOAL), sub=sub, goal=g, third=np.full(n, DEEP))
            return out
        elif name == "c_axis":     # (x, y) the goal's, bit for bit: rad == 0
            g = self.far_goal(n).astype(np.float32).astype(np.float64)
            q = np.concatenate([g, np.full((n, 1), hl)], 1)
            u, rows, out["goal"] = np.stack([z3, z3, z3 + 1], 1), ROW_GOAL, g
        else:
            raise KeyError(name)
        out.update(bp=q + rd[:, None] * u, u=u, rows=np.full(n, rows), primary=np.full(n, rows))
        return out

    def n_inside(self, slot, out):
        """the centre inside the net (nout == 0): by s % 3 within 0.09 m of the top so that the z face is the nearest, lower so that an
        x face is (slots 1 and 4: x = +0.0 and x = -0.0), within 0.09 m of a y end. Slot 0 ties z with x (>=: z), slot 7 x with y (x)."""
        rng, n, nh = self.rng, len(slot), self.nh
        sub = slot % 3
        t = rng.uniform(0.005, 0.09, n)                            # depth under the winning face
        inner = rng.uniform(0.0, 0.95, n) * (nh[0] - t)            # |x| that keeps the x faces farther than t
        sx, sy = self.sign(n), self.sign(n)
        top = np.stack([sx * inner, rng.uniform(-6.2, 6.2, n), nh[2] - t], 1)
        mid = np.stack([rng.uniform(-nh[0], nh[0], n), rng.uniform(-6.2, 6.2, n), rng.uniform(0.06, 0.38, n)], 1)
        end = np.stack([sx * inner, sy * (nh[1] - t), rng.uniform(0.06, 0.38, n)], 1)
        bp = np.where(sub[:, None] == 0, top, np.where(sub[:, None] == 1, mid, end))
        hx, hy = float(np.float32(nh[0])), float(np.float32(nh[1]))
        bp[slot == 1, 0], bp[slot == 4, 0] = 0.0, -0.0
        tie_z, tie_x = slot == 0, slot == 7
        bp[tie_z] = np.stack([np.full(n, hx - 0.03125), bp[:, 1], np.full(n, nh[2] - 0.03125)], 1)[tie_z]   # sz == sx == -1/32 exactly in float32
        bp[tie_x] = np.stack([np.full(n, -(hx - 0.03125)), np.full(n, hy - 0.03125), bp[:, 2]], 1)[tie_x]   # sx == sy == -1/32, x < 0
        face = np.where(tie_x, 1, sub)                             # 0: z face, 1: x face, 2: y face (slot 7 % 3 == 1 already)
        u = np.stack([np.where(rng.random(n) < 0.5, -1.0, 1.0), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n)], 1)   # a flat shot through the net
        out.update(bp=bp, u=u / np.linalg.norm(u, axis=1, keepdims=True), rows=np.full(n, ROW_NET), primary=np.full(n, ROW_NET), sub=face, third=np.full(n, DEEP))
        return out

    def racket_around(self, out):
        """helpers.racket_contact_states' shell recipe around a given ball: candidates (scale, orientation, the ball's place in the
        racket's frame) drawn as there, kept where the racket's COM comes to lie 0.52 .. 0.75 x scale above the court -- at least its
        reach, so that no hull vertex is under the court. That leaves poses with the handle's end pointing down at the ball, and the
        recipe's shell is a box around a much narrower handle: one kept candidate in twenty touches the ball. Even slots therefore try up
        to 48 kept candidates and take the first that the float32 oracle's query_racket calls a hit; odd slots take their first (a racket
        close by that mostly does not touch)."""
        from oracle import query_racket
        rng, p, bp = self.rng, self.p, out["bp"]
        n, tries = len(bp), 48
        ht, r = float(p.racket_half_thick), float(p.ball_radius)
        pad = r + 0.004
        pool = []
        have = 0
        while have < n * tries:
            m = 65536
            scale = rng.uniform(1.0, 3.0, m) if self.kind != ENV_SWING else np.ones(m)
            q = rng.normal(size=(m, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
            loc = np.stack([rng.uniform(-(ht * scale + pad), ht * scale + pad), rng.uniform(-0.16 * scale - pad, 0.16 * scale + pad),
                            rng.uniform(-0.51 * scale - pad, 0.21 * scale + pad)], 1)
            k = rng.integers(0, 3, m); sgn = np.where(rng.random(m) < 0.5, -1.0, 1.0); shell = rng.random(m) < 0.67
            ext = np.stack([ht * scale, 0.15 * scale, np.where(sgn > 0, 0.197, 0.5) * scale], 1)
            idx = np.arange(m)
            loc[idx[shell], k[shell]] = (sgn * (ext[idx, k] + r + rng.uniform(-0.004, 0.001, m)))[shell]
            off = _rot(q, loc)
            h = (0.04 - off[:, 2]) / scale                          # (the balls lie 0.035 .. 0.039 above z = 0)
            ok = (h >= 0.525) & (h <= 0.745)
            pool.append((scale[ok], q[ok], off[ok]))
            have += int(ok.sum())
        scale, q, off = (np.concatenate(x) for x in zip(*pool))
        rp, qq, sc = np.zeros((n, 3)), np.zeros((n, 4)), np.ones(n)
        pq = p.copy()
        for i in range(n):
            cand = np.arange(i * tries, (i + 1) * tries)
            pick = cand[0]
            if i % 2 == 0:
                for j in cand:
                    pq.racket_scale = float(scale[j])
                    if query_racket(pq, (bp[i] - off[j]).astype(np.float32), q[j].astype(np.float32), bp[i].astype(np.float32), "f32")[0]:
                        pick = j
                        break
            rp[i], qq[i], sc[i] = bp[i] - off[pick], q[pick], scale[pick]
        out.update(racket_pos=rp, racket_quat=qq, racket_scale=sc, racket_vel=rng.uniform(-4, 4, (n, 3)), racket_angvel=rng.uniform(-6, 6, (n, 3)))
        out["rows"] = out["rows"] | ROW_RACKET


_CACHE = {}


def _build(kind, rng=None):
    """the blocked batch + the extras: dict of per-lane arrays [64 R + 37]; rng=None: default_rng(SEED), built once and shared"""
    shared = rng is None
    if shared and kind in _CACHE:
        return _CACHE[kind]
    rng = np.random.default_rng(SEED) if shared else rng
    D = _Draw(kind, rng)
    names = REGIONS[kind]
    lanes = [(k, s) for k in range(len(names)) for s in range(LANES)] + [((7 * i + 3) % len(names), (5 * i + 2) % LANES) for i in range(EXTRA)]
    region, slot = np.array([k for k, _ in lanes]), np.array([s for _, s in lanes])
    n = len(lanes)
    park = RACKET_PARK[kind]
    f = dict(bp=np.zeros((n, 3)), u=np.zeros((n, 3)), rows=np.zeros(n, np.int64), primary=np.zeros(n, np.int64), sub=np.zeros(n, np.int64),
             third=np.zeros(n, np.int64), goal=D.far_goal(n), racket_pos=np.tile(park, (n, 1)), racket_quat=np.tile((0.0, 0.0, 0.0, 1.0), (n, 1)),
             racket_scale=np.ones(n), racket_vel=np.zeros((n, 3)), racket_angvel=np.zeros((n, 3)), speed=rng.uniform(0.0, 25.0, n))
    for k, name in enumerate(names):
        for part in (np.flatnonzero((region == k) & (np.arange(n) < n - EXTRA)), np.flatnonzero((region == k) & (np.arange(n) >= n - EXTRA))):
            if len(part):
                for key, v in D.region(name, slot[part]).items():
                    f[key][part] = v
    # velocity: towards the shape (one lane in eight separates), a fifth of the speed across; `high` flies anywhere
    across = rng.normal(size=(n, 3))
    across -= (across * f["u"]).sum(1, keepdims=True) * f["u"] / np.maximum((f["u"] ** 2).sum(1, keepdims=True), 1e-30)
    across /= np.linalg.norm(across, axis=1, keepdims=True)
    towards = np.where(slot % 8 == 7, 1.0, -1.0)
    f["bv"] = f["speed"][:, None] * (towards[:, None] * f["u"] + 0.2 * rng.uniform(0, 1, (n, 1)) * across)
    under = region == names.index("g_under")
    f["bv"][under & (slot % 8 != 7), 2] = np.abs(f["bv"][under & (slot % 8 != 7), 2])   # v_z > 0 under the court
    f["bw"] = rng.uniform(-60, 60, (n, 3))
    f["init_dist"] = rng.uniform(8, 20, n)
    f["steps"] = rng.integers(0, 24, n)
    f.update(region=region, slot=slot)
    if shared:
        _CACHE[kind] = f
    return f


def lane_order(kind, order):
    """lane -> index into the blocked batch"""
    R = len(REGIONS[kind])
    m = R * LANES
    if order == "blocked":
        head = np.arange(m)
    elif order == "interleaved":   # lane i holds region i mod R (its slot i // R)
        i = np.arange(m)
        head = (i % R) * LANES + i // R
    else:
        raise ValueError(order)
    return np.concatenate([head, np.arange(m, m + EXTRA)])


def static_contact_states(kind, order="blocked", rng=None, step_count=None):
    """(words [W, n] uint32, done [n], region [n] (index into names), names). rng: None = default_rng(SEED), the batch every test
    shares. step_count (SwingRacket): None = random in 0 .. 23, or a constant; Tennisbot's is 50."""
    f, perm = _build(kind, rng), lane_order(kind, order)
    fields = dict(racket_pos=f["racket_pos"][perm], racket_quat=f["racket_quat"][perm], racket_vel=f["racket_vel"][perm],
                  racket_angvel=f["racket_angvel"][perm], ball_pos=f["bp"][perm], ball_vel=f["bv"][perm], ball_angvel=f["bw"][perm])
    if kind == ENV_SWING:
        fields.update(goal=f["goal"][perm], spawn_pos=(9, 0, 0.6), init_dist=f["init_dist"][perm],
                      step_count=f["steps"][perm] if step_count is None else int(step_count))
    else:
        fields.update(shoot_force=(30, 0, 20), step_count=50, racket_scale=f["racket_scale"][perm])
    words, done = make_words(kind, len(perm), **fields)
    return words, done, f["region"][perm].copy(), list(REGIONS[kind])


def static_contact_labels(kind, order="blocked"):
    """what the builder intended, per lane: rows (ROW_* bits the label holds), primary (the shape the distance rule was applied to),
    third (DEEP / SHALLOW / GRAZE of that distance; -1: no contact intended), sub (the region's sub-case), slot"""
    f, perm = _build(kind), lane_order(kind, order)
    return {k: f[k][perm].copy() for k in ("rows", "primary", "third", "sub", "slot", "region")}
