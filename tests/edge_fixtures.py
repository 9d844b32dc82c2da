"""What the SAC and the TQC edge fixtures share (tests/test_sac_edges_reference.py, tests/test_tqc_edges_reference.py and the two
GPU modules built on them): the regimes a trained policy reaches and torch's default initialisation never does.

Every fixture starts from the existing one (test_sac_reference.fixture / test_tqc_reference.fixture: nets, pool of 4096 candidate
transitions, critic, target, log_ent_coef), changes the actor's two heads only (for `clamp` the noise scale too) and keeps rows by
the same seeded rejection:

  clamp  log_std.weight x 60, log_std.bias = -9, both noise arrays x 0.3: the clamp of log_std binds below -20 and above 2 in
         about a fifth of the entries each. A row is kept if every raw log_std of both actor passes is KINK_RAW away from -20 AND
         from 2, on either side of each, and |g| <= 4 (no saturation: the float32 twin stays as sharp as in the existing fixtures).
  deep   the ODD rows of mu.weight and the odd entries of mu.bias x 1000: the squash is saturated beyond doubt in the odd columns
         of every row. Kept: log_std KINK_RAW inside the clamp, |g| <= 4 in every even column, |g| >= 18 in every odd one. At
         |g| >= 18, 1 - tanh(g)^2 < 1e-15 in float64 and exactly 0 in float32: both agree that the squash term is log(1e-6) and
         that nothing flows back through the column, so the twin error does not inflate.
  band   all of mu.weight and mu.bias x 60, no bound on |g|: the transition zone 4 < |g| < 18, where float32 itself is imprecise
         (1 - a a carries an absolute error of 6e-8 against the 1e-6 of the epsilon). THIS FIXTURE CATCHES ONLY GROSS FAILURES
         (a NaN, an unclamped action, a wrong sign): its twin error of logp is about 0.1 and of the gradients about 5e-3.

Every fixture also asks |z| >= KINK of every hidden pre-activation of the eight passes, and SAC |Q1 - Q2|(s, a~) >= KINK_Q. The
margins are per fixture, at least 100 x the float32-twin error MEASURED on the fixture's own pool (check_fixture asserts that;
for `deep` over the pool's candidates that pass the conditions on log_std and g: test_sac_edges_reference's docstring says why).

The kept rows are ORDERED (none is dropped) so that the first 17, 65 and 257 of them each hold, in the pass on s and in the pass
on s', what the fixture is for (`coverage`), and so that rows 0 and 256 hold it between the two of them: index_vector's
out-of-range entries clamp to exactly these two rows, so every batch the GPU tests draw from the first 257 rows holds it too.

`Mutant`: the float32 twin of the actor's forward pass and of the actor loss's gradient with ONE line changed. The unchanged
evaluation is the reference's own float32 twin bit for bit (asserted by the test modules), so a mutant differs by that line alone.
"""
import numpy as np

import ppo_reference as ref
from policy_reference import LN_SQRT_2PI

FIXTURES = ("clamp", "deep", "band")
SIZES = (17, 65, 257)       # one past the 16-row tile, a workgroup's 64 rows, the 256-thread blocks of the row kernels
N_ROWS = 257
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
G_MAX, G_SATURATED = 4.0, 18.0
LOG_STD_FACTOR, LOG_STD_BIAS, NOISE_FACTOR = 60.0, -9.0, 0.3      # clamp
DEEP_FACTOR, BAND_FACTOR = 1000.0, 60.0
MUTANTS = {"clamp": ("grad_not_zeroed", "grad_zeroed_below_only", "grad_zeroed_above_only", "no_low_clamp"), "deep": ("softplus_squash", "no_epsilon"), "band": ()}


class Algo:
    """what differs between SAC and TQC: `mod` the reference (sac_reference / tqc_reference), `base` the module of the existing
    fixtures (its fixture() and parts()), whether the min of two critics is a kink"""

    def __init__(self, name, mod, base, qgap):
        self.name, self.mod, self.base, self.qgap = name, mod, base, qgap

    def critic_da(self, PCc, obs, pi, dtype):
        """(the actor loss's gradient with respect to a~ [B, A], the critics' term of the loss per row [B])"""
        m, dt = self.mod, np.dtype(dtype).type
        O, B = pi.x.shape[1], dt(pi.a.shape[0])
        c = [m.critic_forward(PCc, q, m.cat(obs, pi.a, dtype), dtype) for q in (0, 1)]
        da = np.zeros_like(pi.a)
        if self.qgap:          # SAC: -1 / B into the smaller critic, the first on a tie
            first = c[0].q <= c[1].q
            term = np.where(first, c[0].q, c[1].q)
            dqs = [np.where(mask, dt(-1) / B, dt(0)).astype(dtype) for mask in (first, ~first)]
        else:                  # TQC: the mean over 2 x 25 quantiles
            n = dt(2 * c[0].q.shape[1])
            term = np.concatenate([p.q for p in c], 1).sum(1, dtype=dtype) / n
            dqs = [np.full_like(p.q, dt(-1) / (n * B)) for p in c]
        for q in (0, 1):
            da = da + m._critic_backward(PCc, q, c[q], dqs[q])[:, O:]
        return da, term


class Fixture:
    pass


def side(raw):
    """the clamp's state, three-valued: -1 bound below, +1 bound above, 0 unbound"""
    return (raw > LOG_STD_MAX).astype(int) - (raw < LOG_STD_MIN).astype(int)


def edge_distance(raw):
    """per entry: the distance of a raw log_std from the nearer clamp edge, on whichever side of it"""
    return np.minimum(np.abs(raw - LOG_STD_MIN), np.abs(raw - LOG_STD_MAX))


def build(algo, kname, which, kink, kink_raw, kink_q=None):
    """the fixture `which` of env kind `kname`: .actor (the changed heads), the base fixture's critic, target, pool and log_ent_coef,
    .parts64 / .parts32 over the pool, .keep (the pool's rows that pass, in pool order) and .rows (the same rows, ordered)"""
    b = algo.base.fixture(kname)
    f = Fixture()
    for k in ("kind", "O", "A", "critic", "target", "obs", "next_obs", "action", "reward", "done", "log_ent_coef"):
        setattr(f, k, getattr(b, k))
    f.which, f.kname = which, kname
    f.actor = {k: v.copy() for k, v in b.actor.items()}
    f.eps_pi, f.eps_next = b.eps_pi, b.eps_next
    if which == "clamp":
        f.actor["log_std.weight"] = (f.actor["log_std.weight"] * np.float32(LOG_STD_FACTOR)).astype(np.float32)
        f.actor["log_std.bias"] = np.full_like(f.actor["log_std.bias"], LOG_STD_BIAS)
        f.eps_pi, f.eps_next = ((e * np.float32(NOISE_FACTOR)).astype(np.float32) for e in (b.eps_pi, b.eps_next))
    elif which == "deep":
        for k in ("mu.weight", "mu.bias"):
            f.actor[k][1::2] = (f.actor[k][1::2] * np.float32(DEEP_FACTOR)).astype(np.float32)
    elif which == "band":
        for k in ("mu.weight", "mu.bias"):
            f.actor[k] = (f.actor[k] * np.float32(BAND_FACTOR)).astype(np.float32)
    else:
        raise ValueError(which)
    f.kink, f.kink_raw, f.kink_q = kink, kink_raw, kink_q
    f.parts64, f.parts32 = (algo.base.parts(f, f.actor, f.critic, f.target, dt) for dt in (np.float64, np.float32))
    f.keep = np.nonzero(passes(algo, f, f.parts64))[0]
    f.rows = ordered(f, coverage(f, f.parts64))
    return f


def passes(algo, f, p, kinks=True):
    """per row of the passes p = (actor passes, critic passes, the actor-loss result): does it meet the fixture's conditions;
    kinks=False: the conditions on log_std and g alone, without the margins of the ReLUs and of the critic minimum"""
    actors, critics, ag = p
    ok = np.ones(len(actors[0].g), bool)
    if kinks:
        ok &= np.min([np.minimum(np.abs(q.z1).min(1), np.abs(q.z2).min(1)) for q in actors + critics], 0) >= f.kink
    if kinks and algo.qgap:
        ok &= np.abs(ag.c[0].q - ag.c[1].q) >= f.kink_q
    for q in actors:
        g = np.abs(q.g)
        if f.which == "clamp":
            ok &= (edge_distance(q.raw).min(1) >= f.kink_raw) & (g.max(1) <= G_MAX)
        else:
            ok &= np.minimum(q.raw - LOG_STD_MIN, LOG_STD_MAX - q.raw).min(1) >= f.kink_raw
        if f.which == "deep":
            ok &= (g[:, 0::2].max(1) <= G_MAX) & (g[:, 1::2].min(1) >= G_SATURATED)
    return ok


def coverage(f, p):
    """name -> per row of the passes p: the row holds an entry of that sort. What every prefix and, but for band's zones, every
    GPU batch must contain (PAIRED: the sorts that rows 0 and N_ROWS - 1 hold between them)."""
    out = {"terminal": f.done != 0, "not terminal": f.done == 0}
    for name, q in zip(("s", "s'"), p[0]):
        g = np.abs(q.g)
        if f.which == "clamp":
            s = side(q.raw)
            out.update({name + " bound below": (s < 0).any(1), name + " bound above": (s > 0).any(1), name + " unbound": (s == 0).any(1)})
        elif f.which == "deep":
            out.update({name + " beyond 45": (g > 45.0).any(1), name + " beyond 89": (g > 89.0).any(1)})
        else:
            out.update({name + " |g| <= 4": (g <= 4.0).any(1), name + " 4 < |g| <= 9": ((g > 4.0) & (g <= 9.0)).any(1), name + " 9 < |g| <= 45": ((g > 9.0) & (g <= 45.0)).any(1)})
    if f.which == "deep":
        # a saturated column whose float64 1 - a a is not yet exactly 0 (|g| < 19.06): the reference gradient of the odd mu rows is
        # then tiny but not 0, and the twin scale of those tensors is a number and not 0 / 0
        a = p[0][0].a[:, 1::2]
        out["s saturated, 1 - a a > 0 in float64"] = (1.0 - a * a > 0.0).any(1)
    return out


def paired(f, name):
    """is `name` a sort of entry that rows 0 and N_ROWS - 1 must hold between them: all but band's zones of |g| (Tennisbot's two
    columns times two passes times two rows are eight entries for six zones and the two ends of `done`)"""
    return f.which != "band" or "terminal" in name


def ordered(f, cov):
    """f.keep reordered, no row dropped: row 0 and row N_ROWS - 1 hold every paired sort of entry of `cov` between them, and the
    rows after row 0 are a greedy cover of `cov`, so that the first 17 rows hold every sort as well"""
    keep = list(f.keep)
    C = np.stack([cov[k][f.keep] for k in cov], 1)            # [kept rows, sorts]
    P = C[:, [paired(f, k) for k in cov]]
    if len(keep) < N_ROWS:
        return np.asarray(keep)
    first = last = None
    for i in np.argsort(-P.sum(1), kind="stable"):
        rest = np.nonzero((P | P[i]).all(1))[0]
        rest = rest[rest != i]
        if len(rest):
            first, last = int(i), int(rest[0])
            break
    if first is None:
        raise AssertionError("%s %s: no two kept rows hold %s between them" % (f.which, f.kname, [k for k in cov if paired(f, k)]))
    taken, cover, have = {first, last}, [], C[first].copy()
    while not have.all():
        gain = (C & ~have).sum(1)
        gain[list(taken)] = 0
        i = int(np.argmax(gain))
        if gain[i] == 0:
            raise AssertionError("%s %s: no kept row holds %s" % (f.which, f.kname, [k for k, h in zip(cov, have) if not h]))
        cover.append(i); taken.add(i); have |= C[i]
    assert len(cover) + 1 <= SIZES[0] - 1
    order = [first] + cover + [i for i in range(len(keep)) if i not in taken]
    order.insert(N_ROWS - 1, last)
    assert sorted(order) == list(range(len(keep)))
    return f.keep[np.asarray(order)]


def holds_every_sort(f, rows, paired_only=False):
    """the sorts of entry of coverage() (paired_only: the paired ones) that the pool rows `rows` do NOT hold (empty: all held)"""
    cov = coverage(f, f.parts64)
    return [k for k, v in cov.items() if not v[rows].any() and (paired(f, k) or not paired_only)]


def index_vector(N, m, seed):
    """test_gpu_sac.index_vector / test_gpu_tqc.index_vector (the two are the same function), restated here so that the CPU modules
    can see the rows a GPU batch will hold without importing a GPU module; the GPU modules assert that it is theirs"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, m).astype(np.int64)
    if m > 2:
        idx[0] = idx[m - 1]
        idx[1], idx[m // 2] = -5, N + 7
    elif m == 2:
        idx[0], idx[1] = -3, N + 2
    return idx, np.clip(idx, 0, N - 1)


SEEDS = {"forward": 100, "gradient": 300, "step": 77}


def gpu_rows(f, what, m):
    """(the index vector, the pool rows it selects) of the GPU test `what` at batch m over the fixture's first N_ROWS rows"""
    idx, clamped = index_vector(N_ROWS, m, SEEDS[what] + m)
    return idx, f.rows[:N_ROWS][clamped]


# ---------------------------------------------------------------------------------------------------------------------- mutants
class Mutant:
    """the actor's forward pass and the actor loss with its gradient, evaluated in `dtype` with one line changed:
      grad_not_zeroed          (i)   the log_std gradient is not zeroed where the clamp binds
      grad_zeroed_below_only   (ii)  ... is zeroed only below -20
      grad_zeroed_above_only   (iii) ... is zeroed only above 2
      no_low_clamp             (iv)  the forward pass does not clamp on the low side
      softplus_squash          (v)   the squash term of logp is 2 (log 2 - g - softplus(-2 g)), log(1 - tanh(g)^2) without the epsilon
      no_epsilon               (vi)  the gradient's one / (one + 1e-6) is written one / one
    None: no line changed."""

    def __init__(self, algo, which=None):
        self.algo, self.which = algo, which

    def forward(self, PA, obs, eps, dtype):
        m, dt = self.algo.mod, np.dtype(dtype).type
        P, x, eps = m.cast(PA, dtype), np.asarray(obs).astype(dtype), np.asarray(eps).astype(dtype)
        z1 = x @ P["latent_pi.0.weight"].T + P["latent_pi.0.bias"]
        h1 = m._relu(z1)
        z2 = h1 @ P["latent_pi.2.weight"].T + P["latent_pi.2.bias"]
        h2 = m._relu(z2)
        mu = h2 @ P["mu.weight"].T + P["mu.bias"]
        raw = h2 @ P["log_std.weight"].T + P["log_std.bias"]
        if self.which == "no_low_clamp":
            ls = np.minimum(raw, dt(LOG_STD_MAX))
        else:
            ls = np.clip(raw, dt(LOG_STD_MIN), dt(LOG_STD_MAX))
        g = mu + np.exp(ls) * eps
        a = np.tanh(g)
        gauss = (dt(-0.5) * eps * eps - ls - dt(LN_SQRT_2PI)).sum(-1, dtype=dtype)
        if self.which == "softplus_squash":
            squash = (dt(2) * (dt(np.log(2.0)) - g - np.logaddexp(dt(0), dt(-2) * g))).sum(-1, dtype=dtype)
        else:
            squash = np.log(dt(1) - a * a + dt(m.SQUASH_EPS)).sum(-1, dtype=dtype)
        return m.Pass(x=x, eps=eps, z1=z1, h1=h1, z2=z2, h2=h2, mu=mu, raw=raw, ls=ls, g=g, a=a, logp=gauss - squash)

    def loss_and_grads(self, PA, PC, log_ent_coef, obs, eps, dtype):
        """(the gradient over ACTOR_NAMES, {loss, mean_logp, ent_grad}, the actor's pass)"""
        m, dt = self.algo.mod, np.dtype(dtype).type
        PAc, PCc = m.cast(PA, dtype), m.cast(PC, dtype)
        pi = self.forward(PAc, obs, eps, dtype)
        A, B = pi.a.shape[1], dt(pi.a.shape[0])
        alpha = np.exp(dt(log_ent_coef))
        da, term = self.algo.critic_da(PCc, obs, pi, dtype)
        loss = (alpha * pi.logp - term).sum(dtype=dtype) / B
        mean_logp = pi.logp.sum(dtype=dtype) / B
        ent_grad = -((pi.logp + dt(-A)).sum(dtype=dtype) / B)
        cc = alpha / B
        one = dt(1) - pi.a * pi.a
        if self.which == "no_epsilon":
            with np.errstate(invalid="ignore"):
                dg = da * one + cc * ((dt(2) * pi.a) * one / one)
        else:
            dg = da * one + cc * ((dt(2) * pi.a) * one / (one + dt(m.SQUASH_EPS)))
        dmu = dg
        below, above = pi.raw < dt(LOG_STD_MIN), pi.raw > dt(LOG_STD_MAX)
        bound = {"grad_not_zeroed": np.zeros_like(below), "grad_zeroed_below_only": below, "grad_zeroed_above_only": above}.get(self.which, below | above)
        dls = np.where(bound, dt(0), dg * (np.exp(pi.ls) * pi.eps) - cc).astype(dtype)
        g = {}
        g["mu.weight"], g["mu.bias"] = dmu.T @ pi.h2, dmu.sum(0, dtype=dtype)
        g["log_std.weight"], g["log_std.bias"] = dls.T @ pi.h2, dls.sum(0, dtype=dtype)
        dh2 = dmu @ PAc["mu.weight"] + dls @ PAc["log_std.weight"]
        dz2 = dh2 * (pi.z2 > 0)
        g["latent_pi.2.weight"], g["latent_pi.2.bias"] = dz2.T @ pi.h1, dz2.sum(0, dtype=dtype)
        dz1 = (dz2 @ PAc["latent_pi.2.weight"]) * (pi.z1 > 0)
        g["latent_pi.0.weight"], g["latent_pi.0.bias"] = dz1.T @ pi.x, dz1.sum(0, dtype=dtype)
        return {k: g[k] for k in m.ACTOR_NAMES}, {"loss": loss, "mean_logp": mean_logp, "ent_grad": ent_grad}, pi


def odd_mu(grads):
    """the gradient of the odd rows of the mu head, as tensors of their own: the saturated columns of `deep`"""
    return {"mu.weight[1::2]": np.asarray(grads["mu.weight"])[1::2], "mu.bias[1::2]": np.asarray(grads["mu.bias"])[1::2]}


def log_std_head(grads):
    return {k: grads[k] for k in ("log_std.weight", "log_std.bias")}


def checked(f, grads, stats, pi):
    """every tensor the GPU tests hold to the reference on the actor's side, as one dict"""
    out = dict(grads)
    out.update({k: np.asarray(v, np.float64) for k, v in stats.items()})
    out.update({"a": pi.a, "logp": pi.logp})
    if f.which == "deep":
        out.update(odd_mu(grads))
    return out


def mutant_ratio(algo, f, rows, which):
    """the largest distance, in float32-twin errors, of any tensor the GPU tests check from the float64 reference when the float32
    evaluation is the mutant `which` on the pool rows `rows`; (that ratio, its tensor's name). The unchanged twin is asserted to
    be the reference's own."""
    obs, eps = f.obs[rows], f.eps_pi[rows]
    want, twin, got = (checked(f, *Mutant(algo, w).loss_and_grads(f.actor, f.critic, f.log_ent_coef, obs, eps, dt))
                       for w, dt in ((None, np.float64), (None, np.float32), (which, np.float32)))
    ratios = ref.tensor_ratios(got, want, twin)
    worst = max(ratios, key=ratios.get)
    return ratios[worst], worst


def twin_is_the_references(algo, f, rows):
    """Mutant(None) in float32 and in float64 against mod.actor_loss_and_grads: the same bits"""
    obs, eps = f.obs[rows], f.eps_pi[rows]
    for dt in (np.float64, np.float32):
        grads, stats, pi = Mutant(algo).loss_and_grads(f.actor, f.critic, f.log_ent_coef, obs, eps, dt)
        ag = algo.mod.actor_loss_and_grads(f.actor, f.critic, f.log_ent_coef, obs, eps, dt)
        same = all(np.array_equal(grads[k], ag.grads[k]) for k in grads) and np.array_equal(pi.a, ag.pi.a) and np.array_equal(pi.logp, ag.pi.logp)
        same = same and stats["loss"] == ag.loss and stats["mean_logp"] == ag.mean_logp and stats["ent_grad"] == ag.ent_grad
        if not same:
            return False
    return True


def twin_errors(f, rows=slice(None)):
    """measured on the pool (or its rows `rows`): the float32-twin error of (the hidden pre-activations, Q, the raw log_std)"""
    (a64, c64, _), (a32, c32, _) = f.parts64, f.parts32
    z = max(max(np.abs(p.z1[rows] - q.z1[rows]).max(), np.abs(p.z2[rows] - q.z2[rows]).max()) for p, q in zip(a64 + c64, a32 + c32))
    q = max(np.abs(p.q[rows] - q.q[rows]).max() for p, q in zip(c64, c32))
    raw = max(np.abs(p.raw[rows] - q.raw[rows]).max() for p, q in zip(a64, a32))
    return z, q, raw


def same_sides(algo, f, rows):
    """the float64 run and the float32 twin on the pool rows `rows`: the same side of every ReLU of the eight passes, of the
    critic minimum (SAC) and of both clamp edges (the clamp's state three-valued)"""
    (a64, c64, g64), (a32, c32, g32) = f.parts64, f.parts32
    ok = all(np.array_equal(p.z1[rows] > 0, q.z1[rows] > 0) and np.array_equal(p.z2[rows] > 0, q.z2[rows] > 0) for p, q in zip(a64 + c64, a32 + c32))
    ok = ok and all(np.array_equal(side(p.raw[rows]), side(q.raw[rows])) for p, q in zip(a64, a32))
    if algo.qgap:
        ok = ok and np.array_equal(g64.first[rows], g32.first[rows])
    return ok


# ------------------------------------------------------------------------------------- what both CPU modules assert of a fixture
def check_fixture(algo, f, pool):
    """the margins against the measured twin errors, the kept rows and their order, the sides of every kink, the regime's shares"""
    tag = "%s %s %s" % (algo.name, f.which, f.kname)
    assert len(f.parts64[0][0].g) == pool
    z_pool, q_pool, raw_err = twin_errors(f)
    z_err, q_err = z_pool, q_pool
    if f.which == "deep":      # over the candidates that pass the conditions on log_std and g (the module docstrings say why)
        cand = np.nonzero(passes(algo, f, f.parts64, kinks=False))[0]
        assert len(cand) >= pool // 2
        z_err, q_err, _ = twin_errors(f, cand)
        assert G_SATURATED - 100.0 * max(np.abs(p.g - q.g)[np.abs(p.g) < 2.0 * G_SATURATED].max() for p, q in zip(f.parts64[0], f.parts32[0])) > 9.0, \
            "the twin's g near the |g| >= 18 rule is not on the saturated side beyond doubt"
    print("%s: float32-twin error: pre-activations %.3g (pool-wide %.3g), Q %.3g (pool-wide %.3g), raw log_std %.3g; %d of %d rows kept"
          % (tag, z_err, z_pool, q_err, q_pool, raw_err, len(f.keep), pool))
    assert 100.0 * z_err <= f.kink and 100.0 * raw_err <= f.kink_raw
    if algo.qgap:
        assert 100.0 * q_err <= f.kink_q
    assert len(f.keep) >= N_ROWS, "%s: the pool leaves %d rows, %d are needed" % (tag, len(f.keep), N_ROWS)
    assert sorted(f.rows) == sorted(f.keep) and len(set(f.rows)) == len(f.rows), "ordering dropped or repeated a row"
    assert passes(algo, f, f.parts64)[f.rows].all()
    # the conditions hold on a fresh evaluation of the first N_ROWS rows alone (what the GPU tests compare against)
    rows = f.rows[:N_ROWS]
    fresh = algo.base.parts(f, f.actor, f.critic, f.target, np.float64, rows)
    assert passes(algo, f, fresh).all()
    assert 0 < f.done[rows].sum() < N_ROWS
    for n in SIZES:
        missing = holds_every_sort(f, f.rows[:n])
        assert not missing, "%s: the first %d rows hold no entry %s" % (tag, n, missing)
        for what in ("forward", "gradient"):
            missing = holds_every_sort(f, gpu_rows(f, what, n)[1], paired_only=True)
            assert not missing, "%s: the GPU %s batch of %d rows holds no entry %s" % (tag, what, n, missing)
    assert not holds_every_sort(f, gpu_rows(f, "step", 65)[1], paired_only=True)
    assert same_sides(algo, f, f.rows), "%s: the float32 twin took another side of a kink on a kept row" % tag
    assert twin_is_the_references(algo, f, rows[:SIZES[0]]) and twin_is_the_references(algo, f, rows)
    # the regime, over the first N_ROWS rows
    for name, p in zip(("s", "s'"), f.parts64[0]):
        g, s = np.abs(p.g[rows]), side(p.raw[rows])
        share = lambda m: float(np.mean(m))  # noqa: E731
        print("%s, pass on %s: log_std bound below %.3f, above %.3f; |g| <= 4 %.3f, 4..9 %.3f, 9..45 %.3f, > 45 %.3f, > 89 %.3f, largest %.0f"
              % (tag, name, share(s < 0), share(s > 0), share(g <= 4), share((g > 4) & (g <= 9)), share((g > 9) & (g <= 45)), share(g > 45), share(g > 89), g.max()))
        if f.which == "clamp":
            assert share(s < 0) > 0.05 and share(s > 0) > 0.01 and share(s == 0) > 0.3 and g.max() <= G_MAX
            assert edge_distance(p.raw[rows]).min() >= f.kink_raw
        else:
            assert (s == 0).all()
        if f.which == "deep":
            assert g[:, 0::2].max() <= G_MAX and g[:, 1::2].min() >= G_SATURATED and share(g > 45) > 0.3 and share(g > 89) > 0.2
        if f.which == "band":
            assert share(g <= 4) > 0.05 and share((g > 4) & (g <= G_SATURATED)) > 0.2 and share(g > G_SATURATED) > 0.2
    # the twin errors of what the GPU tests compare: as sharp as the existing fixtures for clamp and deep, coarse for band
    want, twin = (checked(f, *Mutant(algo).loss_and_grads(f.actor, f.critic, f.log_ent_coef, f.obs[rows], f.eps_pi[rows], dt)) for dt in (np.float64, np.float32))
    scale = ref.twin_scale(want, twin)
    names = algo.mod.ACTOR_NAMES
    g_err, g_size = max(scale[k] for k in names), max(np.abs(want[k]).max() for k in names)
    print("%s: twin error over %d rows: logp %.3g, gradients %.3g (largest entry %.3g)" % (tag, N_ROWS, scale["logp"], g_err, g_size))
    if f.which != "band":
        assert scale["logp"] <= 1e-3 and g_err <= 1e-4 * g_size
    if f.which == "deep":
        cc = np.exp(f.log_ent_coef) / N_ROWS
        odd = odd_mu(want)
        print("%s: reference gradient of the odd mu rows: at most %.3g = %.3g alpha / B" % (tag, max(np.abs(v).max() for v in odd.values()), max(np.abs(v).max() for v in odd.values()) / cc))
        for k, v in odd.items():
            assert 0.0 < np.abs(v).max() <= 1e-9 * cc * max(1.0, np.abs(f.parts64[0][0].h2[rows]).sum(0).max()), k
        assert (np.abs(twin["a"][:, 1::2]) == 1.0).all(), "the float32 twin's tanh is not exactly +-1 in a saturated column"


def check_mutants(algo, f):
    """every mutant of the fixture more than ref.MULTIPLE twin errors from the float64 reference, at each of SIZES rows: on the
    prefixes of the ordered rows and on the batches the GPU tests draw"""
    for which in MUTANTS[f.which]:
        worst = np.inf
        for n in SIZES:
            batches = {"the first %d rows" % n: f.rows[:n], "the GPU forward batch of %d" % n: gpu_rows(f, "forward", n)[1], "the GPU gradient batch of %d" % n: gpu_rows(f, "gradient", n)[1]}
            for name, rows in batches.items():
                r, tensor = mutant_ratio(algo, f, rows, which)
                assert r > ref.MULTIPLE, "%s %s %s: the mutant %s is %.3g twin errors away on %s (%s): it would pass" % (algo.name, f.which, f.kname, which, r, name, tensor)
                worst = min(worst, r)
        print("%s %s %s: mutant %s: at least %.3g twin errors from the reference" % (algo.name, f.which, f.kname, which, worst))
    assert mutant_ratio(algo, f, f.rows[:N_ROWS], None)[0] <= 1.0      # no line changed: the twin itself
