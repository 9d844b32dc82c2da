"""What the labelled forced states of tests/static_contact_fixtures.py reach, on the oracle alone: conditions on the INPUTS of
tests/test_gpu_static_contacts.py, not measurements of the code under test. That file holds the kernels to the float32 oracle bit
for bit on this batch; this one keeps it from passing vacuously -- every lane's label holds on the oracle's own narrowphase
(query_box / query_goal / query_racket on the initial state), graze lanes split into hit and no-hit, the multi-row regions hold their
rows, and the rows change where the balls end up.

One wording of the fixture's specification is narrowed here on purpose: inside the net the x face's normal follows `x < 0` (what
sphere_vs_box tests), so the lane x = -0.0 gets +1 like x = +0.0 -- the sign bit of a zero does not count."""
import functools

import numpy as np

from oracle import OracleBatch, query_box, query_goal, query_racket
from static_contact_fixtures import EDGE_REGIONS, GRAZE, LANES, REGIONS, ROW_GOAL, ROW_GROUND, ROW_RACKET, static_contact_labels, static_contact_states
from tennisbot_rl_amd.params import COUNTER_NAMES, ENV_SWING, ENV_TENNIS, F_NET, STATE_ROWS, default_params

KINDS = (ENV_TENNIS, ENV_SWING)
STEPS = 8
# the row counts the issue of this batch asks for (lanes of the 64 of a region's block)
TWO_ROWS_AT_LEAST, THREE_ROWS_AT_LEAST, RACKET_AND_STATIC_AT_LEAST = 48, 32, 16


def rows_of(kind, name):
    names = STATE_ROWS[kind]
    return [i for i, nm in enumerate(names) if nm == name]


def altered(params):
    """the twin whose court and goal rows act differently"""
    p = params.copy()
    p.rest_court, p.fric_court, p.rest_goal, p.fric_goal = 0.35, 0.5, 0.4, 0.05
    return p


def without_net(params):
    p = params.copy()
    p.flags &= ~F_NET
    return p


def actions_of(kind, n, steps=STEPS):
    return np.random.default_rng(17).uniform(-1, 1, (steps, n, 2 if kind == ENV_TENNIS else 6)).astype(np.float32)


def run_oracle(kind, params, words, done, actions, precision="f32"):
    """(final words, done byte, counters by name) of the oracle without auto-reset from these words through these actions"""
    ref = OracleBatch(params, kind, words.shape[1], seed=11, precision=precision, threads=8)
    ref.set_state_words(words, done)
    for a in actions:
        ref.step(a)
    w, d = ref.get_state_words()
    c = dict(zip(COUNTER_NAMES, [int(x) for x in ref.counters()]))
    ref.close()
    return w, d, c


@functools.lru_cache(maxsize=None)
def narrowphase(kind, precision="f32"):
    """the oracle's narrowphase on every lane of the blocked batch: rows [n] (ROW_* bits), normal [n, 4, 3] by row, dist [n, 4]"""
    p = default_params()
    words, _, region, names = static_contact_states(kind)
    f = words[:-2].view(np.float32)
    bp, rp, rq = (np.ascontiguousarray(f[rows_of(kind, nm)].T) for nm in ("ball_pos", "racket_pos", "racket_quat"))   # (the queries take raw pointers)
    n = words.shape[1]
    rows, normal, dist = np.zeros(n, np.int64), np.zeros((n, 4, 3)), np.full((n, 4), np.inf)
    gh, nh = [float(x) for x in p.ground_half], [float(x) for x in p.net_half]
    for i in range(n):
        res = [None, query_box(p, gh, bp[i], precision), query_box(p, nh, bp[i], precision), None]
        pr = p.copy()
        if kind == ENV_TENNIS:
            pr.racket_scale = float(f[rows_of(kind, "racket_scale")[0], i])
        res[0] = query_racket(pr, rp[i], rq[i], bp[i], precision)[:3]
        if kind == ENV_SWING:
            g = f[rows_of(kind, "goal"), i]
            res[3] = query_goal(p, float(g[0]), float(g[1]), bp[i], precision)
        for k, h in enumerate(res):
            if h is not None and h[0]:
                rows[i] |= 1 << k
                dist[i, k], normal[i, k] = h[1], h[2]
    return rows, normal, dist


def block(kind, name):
    """the lanes of a region's own 64-lane block"""
    k = REGIONS[kind].index(name)
    return np.arange(k * LANES, (k + 1) * LANES)


def approaching(kind):
    """lanes that hit something and move towards it (v . n < 0 for one of their rows)"""
    words, _, _, _ = static_contact_states(kind)
    bv = words[:-2].view(np.float32)[rows_of(kind, "ball_vel")].T.astype(np.float64)
    rows, normal, _ = narrowphase(kind)
    app = np.zeros(len(rows), bool)
    for k in range(1, 4):
        app |= ((rows >> k) & 1).astype(bool) & ((bv * normal[:, k]).sum(1) < 0.0)
    return app


def census(kind):
    """per region: lanes that hit, and the row sets reached (the table in test_gpu_static_contacts.py's docstring)"""
    rows, _, _ = narrowphase(kind)
    _, _, region, names = static_contact_states(kind)
    out = {}
    for k, name in enumerate(names):
        r = rows[region == k]
        sets = {}
        for x in r:
            key = "".join(c for c, b in zip("RGNC", (1, 2, 4, 8)) if x & b) or "-"
            sets[key] = sets.get(key, 0) + 1
        out[name] = (int((r != 0).sum()), len(r), sets)
    return out


def test_lane_orders_hold_the_same_states():
    for kind in KINDS:
        R = len(REGIONS[kind])
        wb, db, rb, names = static_contact_states(kind, "blocked")
        wi, di, ri, _ = static_contact_states(kind, "interleaved")
        n = wb.shape[1]
        assert n == R * LANES + 37 and n % 64 != 0 and names == REGIONS[kind]
        assert np.array_equal(rb[:R * LANES], np.repeat(np.arange(R), LANES)) and np.array_equal(ri[:R * LANES], np.arange(R * LANES) % R)
        assert np.array_equal(rb[R * LANES:], ri[R * LANES:]) and len(set(rb[R * LANES:].tolist())) > 8
        i = np.arange(R * LANES)
        assert np.array_equal(wi[:, i], wb[:, (i % R) * LANES + i // R]) and np.array_equal(wi[:, R * LANES:], wb[:, R * LANES:])
        if kind == ENV_SWING:
            sc = wb[-2].view(np.int32)
            assert sc.min() == 0 and sc.max() == 23
            assert (static_contact_states(kind, "blocked", step_count=10)[0][-2].view(np.int32) == 10).all()


def test_labels_hold():
    for kind in KINDS:
        rows, normal, dist = narrowphase(kind)
        lab = static_contact_labels(kind)
        words, _, region, names = static_contact_states(kind)
        bx = words[rows_of(kind, "ball_pos")[0]].view(np.float32)
        for i in range(len(rows)):
            name, want, prim, static = names[region[i]], int(lab["rows"][i]), int(lab["primary"][i]), int(rows[i]) & ~ROW_RACKET
            what = "%s lane %d (%s)" % ("Tennisbot" if kind == ENV_TENNIS else "SwingRacket", i, name)
            if lab["third"][i] == GRAZE:   # the graze distance belongs to the primary shape: that row may be missing, the others hold
                assert static | prim == want & ~ROW_RACKET, (what, static, want)
            else:
                assert static == want & ~ROW_RACKET, (what, static, want)
            if not (want & ROW_RACKET):
                assert not (rows[i] & ROW_RACKET), what + ": the parked racket is touched"
            for k in (1, 2, 3):   # the normal classes of the rows that hit
                if not (rows[i] >> k) & 1:
                    continue
                nrm = np.abs(normal[i, k])
                oblique = (1 << k) == prim and name in EDGE_REGIONS
                if oblique:
                    assert (nrm > 0.05).sum() >= (3 if name in ("g_corner", "n_corner") else 2), (what, normal[i, k])
                else:
                    axis_aligned = sorted(nrm.tolist())[:2] == [0.0, 0.0] and nrm.max() == 1.0
                    radial = name in ("c_wall", "c_inside") and k == 3 and nrm[2] == 0.0   # the goal's wall: a horizontal unit vector
                    assert axis_aligned or radial, (what, normal[i, k])
            if name == "n_inside":
                face = int(lab["sub"][i])
                axis = (2, 0, 1)[face]
                assert abs(normal[i, 2, axis]) == 1.0 and dist[i, 2] < -float(default_params().ball_radius), (what, normal[i, 2])
                if face == 1:
                    assert normal[i, 2, 0] == (-1.0 if bx[i] < 0 else 1.0), what
        inside = block(kind, "n_inside")
        assert {int(x) for x in lab["sub"][inside]} == {0, 1, 2}
        zeros = bx[inside][(bx[inside] == 0)]
        assert len(zeros) == 2 and sorted(np.signbit(zeros).tolist()) == [False, True], "x = +0.0 and x = -0.0 are among the x-face lanes"
        if kind == ENV_SWING:   # c_inside: some nearer the cap, some nearer the wall; c_axis: the goal's (x, y) bit for bit
            ci = block(kind, "c_inside")
            assert (np.abs(normal[ci, 3, 2]) == 1.0).sum() >= 16 and (normal[ci, 3, 2] == 0.0).sum() >= 16
            ax = block(kind, "c_axis")
            g = words[rows_of(kind, "goal")][:, ax]
            assert np.array_equal(g, words[rows_of(kind, "ball_pos")[:2]][:, ax])


def test_graze_lanes_split():
    for kind in KINDS:
        rows, _, _ = narrowphase(kind)
        lab = static_contact_labels(kind)
        _, _, region, names = static_contact_states(kind)
        for k, name in enumerate(names):
            g = (region == k) & (lab["third"] == GRAZE)
            if not g.any():
                assert name in ("high", "n_inside", "c_inside"), name
                continue
            hit = (rows[g] & lab["primary"][g]) != 0
            assert hit.any() and (~hit).any(), (name, int(hit.sum()), int(g.sum()))
    # an edge lane with every per-axis separation inside the threshold and no hit (the Euclidean distance decides)
    p = default_params()
    r, thr = float(p.ball_radius), float(p.contact_threshold)
    found = 0
    for kind in KINDS:
        rows, _, _ = narrowphase(kind)
        words, _, region, names = static_contact_states(kind)
        bp = words[rows_of(kind, "ball_pos")].view(np.float32).T.astype(np.float64)
        for name, half in (("g_edge_x", p.ground_half), ("g_edge_y", p.ground_half), ("g_corner", p.ground_half), ("n_tape", p.net_half),
                           ("n_end_edge", p.net_half), ("n_corner", p.net_half)):
            lanes = np.flatnonzero(region == names.index(name))
            sep = np.abs(bp[lanes]) - np.array([float(x) for x in half])[None, :]
            found += int((((sep - r) < thr).all(1) & (rows[lanes] == 0)).sum())
    assert found >= 1


def test_row_counts():
    for kind in KINDS:
        rows, _, _ = narrowphase(kind)
        static = lambda lanes: np.array([bin(int(x) & ~ROW_RACKET).count("1") for x in rows[lanes]])   # noqa: E731
        assert (static(block(kind, "n_foot")) == 2).sum() >= TWO_ROWS_AT_LEAST
        rf = block(kind, "r_foot")
        both = ((rows[rf] & ROW_RACKET) != 0) & (static(rf) >= 1)
        print("%s r_foot: %d lanes hold a racket row with a static row" % ("Tennisbot" if kind == ENV_TENNIS else "SwingRacket", int(both.sum())))
        assert both.sum() >= RACKET_AND_STATIC_AT_LEAST
        if kind == ENV_SWING:
            cw = block(kind, "c_wall")
            on_court = static_contact_labels(kind)["sub"][cw] == 0
            assert (rows[cw][on_court] == (ROW_GROUND | ROW_GOAL)).sum() >= TWO_ROWS_AT_LEAST and on_court.sum() == LANES - 8
            assert (rows[cw][~on_court] == ROW_GOAL).any()
            assert (rows[cw][~on_court] & ROW_GROUND == 0).all()
            assert (static(block(kind, "c_net")) == 3).sum() >= THREE_ROWS_AT_LEAST


@functools.lru_cache(maxsize=None)
def acted(kind):
    """per region of the blocked batch: (lanes that hit and approach, those of them whose final state differs from the twin's) on the
    float32 oracle after 8 steps; the twin: without the net for the regions with a net row, altered court and goal rows for the others"""
    p = default_params()
    words, done, region, names = static_contact_states(kind)
    acts = actions_of(kind, words.shape[1])
    w, _, c = run_oracle(kind, p, words, done, acts)
    w_alt, _, c_alt = run_oracle(kind, altered(p), words, done, acts)
    w_net, _, c_net = run_oracle(kind, without_net(p), words, done, acts)
    assert c["nonfinite_states"] == 0 and c_alt["nonfinite_states"] == 0 and c_net["nonfinite_states"] == 0
    assert np.isfinite(w[:-2].view(np.float32)).all()
    app = approaching(kind)
    out = {}
    for k, name in enumerate(names):
        if name == "high":
            continue
        lanes = (region == k) & app
        twin = w_net if name.startswith("n_") or name in ("c_net", "r_foot") else w_alt
        out[name] = (int(lanes.sum()), int((w[:, lanes] != twin[:, lanes]).any(0).sum()))
    return out, c


def test_the_rows_act():
    for kind in KINDS:
        out, c = acted(kind)
        print("%s: (hit and approach, end elsewhere) %s; counters %s" % ("Tennisbot" if kind == ENV_TENNIS else "SwingRacket", out, c))
        for name, (lanes, moved) in out.items():
            assert lanes >= 24, (name, lanes)
            assert 4 * moved >= 3 * lanes, (name, lanes, moved)
        if kind == ENV_SWING:
            assert c["ball_court_terminations"] > 0 and c["goal_hits"] > 0


def test_the_rolling_rows_act_on_every_region():
    """the extended contact set (racket<->court contact, rolling-friction rows) on the same states: in every contact region at least
    half of the lanes that hit and approach end elsewhere than with the default set -- a rolling row does nothing only to a ball
    without spin about the row's axes, and every ball here spins at up to 60 rad/s about all three"""
    from tennisbot_rl_amd.params import F_DEFAULT, F_RACKET_GROUND, reference_rolling_friction
    for kind in KINDS:
        words, done, region, names = static_contact_states(kind)
        acts = actions_of(kind, words.shape[1])
        w, _, _ = run_oracle(kind, default_params(), words, done, acts)
        wx, _, cx = run_oracle(kind, default_params(flags=F_DEFAULT | F_RACKET_GROUND, **reference_rolling_friction()), words, done, acts)
        assert cx["nonfinite_states"] == 0
        app = approaching(kind)
        out = {name: (int(((region == k) & app).sum()), int(((region == k) & app & (w != wx).any(0)).sum())) for k, name in enumerate(names) if name != "high"}
        print("%s: (hit and approach, end elsewhere with the extended contact set) %s" % ("Tennisbot" if kind == ENV_TENNIS else "SwingRacket", out))
        assert all(2 * moved >= lanes for lanes, moved in out.values()), out


def test_float32_and_float64_agree_on_the_hit_decision():
    for kind in KINDS:
        r32, _, _ = narrowphase(kind)
        r64, _, _ = narrowphase(kind, "f64")
        lab = static_contact_labels(kind)
        differ = r32 != r64
        graze = lab["third"] == GRAZE
        print("%s: float32 and float64 disagree on %d of %d graze lanes (%.1f %%)" % ("Tennisbot" if kind == ENV_TENNIS else "SwingRacket",
              int((differ & graze).sum()), int(graze.sum()), 100.0 * (differ & graze).sum() / graze.sum()))
        assert not (differ & ~graze).any(), np.flatnonzero(differ & ~graze)


def test_census_printout():
    """the table of test_gpu_static_contacts.py's docstring: lanes that hit / lanes, and the row sets reached (R racket, G ground, N net, C goal)"""
    for kind in KINDS:
        for name, (hit, lanes, sets) in census(kind).items():
            print("%-9s %-11s %3d / %3d  %s" % ("Tennisbot" if kind == ENV_TENNIS else "SwingRacket", name, hit, lanes, sets))
        hit_high = census(kind)["high"][0]
        assert hit_high == 0
