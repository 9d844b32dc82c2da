"""What the on-policy learner kernels' edge tests share (tests/test_learner_edges_reference.py on CPU, tests/test_gpu_learner_edges.py
and tests/test_gpu_trpo_edges.py on the device): the regimes tb_ppo_grad, tb_ppo_grad_net, tb_trpo_fvp and tb_trpo_search reach in
training and test_ppo_reference.make_policy / make_rollout never do.

Everything starts from test_ppo_reference.rollout("swing-52-lockstep") / rollout("tennis-70-ragged"): the env kind, the net of
make_policy, the hyper-parameters, the observations and a POOL of 1024 rows drawn from the rollout's T n rows by a seeded permutation.

Weight regimes (both towers; the actions are re-drawn from the changed policy with the rollout's own seed, old_logp is their float64
log-probability + N(0, 0.25), the returns sit near the changed critic):
  saturating  every hidden weight matrix N(0, 2^2): more than half of all hidden activations have |h| > 0.999 (1 - h h cancels)
  overflow    make_policy's weights; first-layer unit 0's bias lifts z to >= 50 on every row, unit 1's bias lowers it to <= -50:
              exp2(2.885 z) is inf / 0 on the device and h must be exactly +-1, dz exactly 0
  log_std     log_std = (-5, 2, -5, 2, ...): the standardised sample is (raw - mu) * 148, a difference of numbers of size 30
Data regimes (make_policy's weights, the rollout's actions):
  all_inactive        old_logp puts every ratio outside [1 - c, 1 + c] on the side where the clipped term is the smaller one
  all_active_outside  the mirror image: every row outside the range and active (the clip changes nothing)
  wide_ratio          log(ratio) uniform over [-20, 20]
  constant_adv        every advantage 0.25; constant_adv_tenth: every advantage float32(0.1)
  offset_adv          advantages 1000 + N(0, OFFSET_SCALE^2), rounded to float32: for the one-pass sums of the statistics pre-pass

Rows are kept by rejection, in pool order, then ORDERED (rows of positive and of negative A_hat alternate, so that short prefixes are
balanced). A row is kept if its float64 ratio is MARGIN = 100 float32-twin errors of that ratio (the pool's largest relative twin
error times the ratio) from both 1 - c and 1 + c and, except with constant advantages, if its pool-normalised |A_hat| is MARGIN
pool twin errors from 0. all_inactive / all_active_outside also drop the rows whose advantage lies in the middle BAND of the
pool's advantages: the side old_logp was built for is the sign of A_hat, which moves with the minibatch's mean. At most half of the
pool may go. The device arrays are the first N_ROWS = 257 kept rows; a GPU batch of B = 17, 129, 257 is an index vector over them
with a repeat and two out-of-range entries (clamped to rows 0 and 256), `gpu_rows`; its seed is the first whose batch is `representative`.

The line search (`search_case`) adds candidates that are not finite: giant steps (NaN rows) and a ratio that overflows to +inf on one
row beside an acceptable KL. The tuned net (`tuned_fixture`) runs log_std, all_inactive and constant advantages on the existing tuned
fixtures and a large-magnitude ReLU regime of its own (`tuned_saturating`).

`Mutant` is the float32 twin of ppo_reference.loss_and_grads, trpo_reference.fvp and trpo_reference.search_table with ONE line
changed (None: no line, bit for bit the reference's twin); `Mutant("fast_tanh")` is the EMULATED twin: tanh by fast_tanh's formula
1 - 2 rcp(exp2(2.885 z) + 1) with +-1 ulp of noise on the exp2 and on the reciprocal.
"""
import numpy as np

import ppo_reference as ref
import trpo_reference as tr
from edge_fixtures import index_vector
from policy_reference import state_dict_arrays
from test_ppo_reference import flat_shard, make_policy, rollout

CASE = {"swing": "swing-52-lockstep", "tennis": "tennis-70-ragged"}
SIZES = (17, 129, 257)      # one past the 16-row tile, one past a wave's half share of 128, one past a workgroup's 256
N_ROWS = 257
POOL = 1024
MARGIN = 100.0
BAND = (0.3, 0.7)           # quantiles of the pool's advantages that all_inactive / all_active_outside leave out
SATURATED = 0.999
OVERFLOW_Z = 50.0
OFFSET, OFFSET_SCALE = 1000.0, 1e-2
DIRECTION_MAX = 4.0
INF_OLD_LOGP = -1000.0
LOG_STD_MOVE = 0.2         # |d log_std| of the line search's first candidate, largest component
WEIGHT_REGIMES = ("saturating", "overflow", "log_std")
DATA_REGIMES = ("all_inactive", "all_active_outside", "wide_ratio", "constant_adv", "constant_adv_tenth", "offset_adv")
REGIMES = WEIGHT_REGIMES + DATA_REGIMES
SEEDS = {"grad": 300, "fvp": 100, "search": 200}
ORDERS = 4
# mutant -> (the fixture that must reject it, the kernel it is a wrong version of)
MUTANTS = {"tanh_ratio_form": ("overflow", "grad"), "stats_float32_one_pass": ("offset_adv", "grad"), "no_adv_epsilon": ("constant_adv", "grad"),
           "clip_above_only": ("all_inactive", "grad"), "fvp_inv_std": ("log_std", "fvp"), "search_old_sigma": ("log_std", "search"),
           "search_e2_single": ("log_std", "search")}
_cache = {}


class Fixture:
    pass


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def logp64(P, obs, act):
    _, mu = tr.mean_of(P, obs)
    zeta = (np.asarray(act, np.float64) - mu) * np.exp(-P["log_std"])
    return (-0.5 * zeta * zeta - P["log_std"] - tr.LN_SQRT_2PI).sum(-1)


def hidden(P, obs, body, head):
    """(hidden activations per layer, first-layer pre-activations) of one tower in float64"""
    hs, _ = ref._tower(ref.cast_params(P, np.float64), body, head, np.asarray(obs, np.float64))
    return hs[1:], np.asarray(obs, np.float64) @ P[body + ".0.weight"].T + P[body + ".0.bias"]


def saturated_share(P, obs):
    h = np.concatenate([a.reshape(-1) for body, head in (("policy_net", "action_net"), ("value_net_body", "value_net")) for a in hidden(P, obs, body, head)[0]])
    return float((np.abs(h) > SATURATED).mean())


def build(kname, which):
    """the fixture `which` of env kind `kname`: .P (float32 values as float64 arrays), .hp, .data = (obs, act, old_logp, adv, returns)
    over the kept rows in their order, .pool_data the same over the whole pool, .keep (pool rows kept, ordered), .kept (their number),
    .ratio_err / .adv_err (the pool's float32-twin errors the margins are multiples of)"""
    if (kname, which) in _cache:
        return _cache[kname, which]
    ro = rollout(CASE[kname])
    f = Fixture()
    f.kname, f.which, f.ro, f.hp, f.kind, f.arch, f.A = kname, which, ro, dict(ro.hp), ro.kind, ro.arch, ro.A
    rng = np.random.default_rng(7000 + 10 * REGIMES.index(which) + list(CASE).index(kname))
    pool = rng.permutation(ro.T * ro.n)[:POOL]
    obs, act, old_logp, adv, ret = (x[pool].copy() for x in flat_shard(ro, ro.gae.adv, ro.gae.returns))
    v_pred = ro.v_pred.reshape(-1)[pool]
    P = {k: v.copy() for k, v in state_dict_arrays(make_policy(ro.arch, ro.kind)).items()}
    if which == "saturating":
        for k in P:
            if k.endswith(".weight") and (k.startswith("policy_net.") or k.startswith("value_net_body.")):
                P[k] = f32(rng.normal(0.0, 2.0, P[k].shape)).astype(np.float64)
    elif which == "overflow":
        for body in ("policy_net", "value_net_body"):
            z = obs.astype(np.float64) @ P[body + ".0.weight"].T
            b = P[body + ".0.bias"]
            b[0], b[1] = np.float32(OVERFLOW_Z + 2.0 - z[:, 0].min()), np.float32(-OVERFLOW_Z - 2.0 - z[:, 1].max())
    elif which == "log_std":
        P["log_std"] = np.resize(np.array([-5.0, 2.0]), ro.A)
    if which in WEIGHT_REGIMES:
        _, mu = tr.mean_of(P, obs)
        noise = np.random.default_rng(sum(map(ord, ro.name))).normal(size=(POOL, ro.A))      # the rollout's own seed
        act = f32(mu + np.exp(P["log_std"]) * noise)
        old_logp = f32(logp64(P, obs, act) + rng.normal(0.0, 0.25, POOL))
        _, value = ref._tower(P, "value_net_body", "value_net", obs.astype(np.float64))
        ret = f32(value[:, 0] + 0.01 * (ret - v_pred))
    else:
        ret = f32(v_pred + 0.01 * (ret - v_pred))            # near the critic: the value gradient at the size of the policy's
    lp = logp64(P, obs, act)
    ok = np.ones(POOL, bool)
    if which in ("all_inactive", "all_active_outside"):
        lo, hi = np.quantile(adv, BAND)
        ok &= (adv < lo) | (adv > hi)
        up = (adv > hi) == (which == "all_inactive")        # all_inactive: ratio > 1 + c where A_hat > 0, < 1 - c where A_hat < 0
        old_logp = f32(lp - np.where(up, 1.0, -1.0) * rng.uniform(0.3, 1.5, POOL))
    elif which == "wide_ratio":
        old_logp = f32(lp - rng.uniform(-20.0, 20.0, POOL))
    elif which == "constant_adv":
        adv = np.full(POOL, 0.25, np.float32)
    elif which == "constant_adv_tenth":
        adv = np.full(POOL, 0.1, np.float32)
    elif which == "offset_adv":
        adv = f32(OFFSET + rng.normal(0.0, OFFSET_SCALE, POOL))
    f.P, f.pool_data = P, (obs, act, old_logp, adv, ret)
    # the kinks: the clip's two edges and the advantage's sign, against the twin error measured on this very pool
    want, twin = (ref.loss_and_grads(P, *f.pool_data, f.hp, dt) for dt in (np.float64, np.float32))
    f.ratio_err = float(np.abs(twin.ratio.astype(np.float64) / want.ratio - 1.0).max())
    c = f.hp["clip_range"]
    ok &= np.minimum(np.abs(want.ratio - (1.0 - c)), np.abs(want.ratio - (1.0 + c))) >= MARGIN * f.ratio_err * want.ratio
    f.constant = which.startswith("constant_adv")
    f.adv_err = 0.0
    if not f.constant:
        f.adv_err = float(np.abs(twin.adv_norm.astype(np.float64) - want.adv_norm).max())
        ok &= np.abs(want.adv_norm) >= MARGIN * f.adv_err
    f.kept, f.pool_adv_norm = int(ok.sum()), want.adv_norm
    keep = np.nonzero(ok)[0]
    pos, neg = list(keep[want.adv_norm[keep] > 0]), list(keep[want.adv_norm[keep] <= 0])
    order = []
    while pos and neg:
        order += [pos.pop(0), neg.pop(0)]
    f.keep = np.asarray(order + pos + neg, np.int64)
    f.data = tuple(x[f.keep] for x in f.pool_data)
    _cache[kname, which] = f
    return f


def representative(run, rows, want):
    """is the twin's error on this batch a fair sample of itself? check_tensors' scale is the twin's error, floored at u max|tensor|.
    A tensor with one or two entries that are sums over the batch's rows can cancel far below the size of its terms, so the floor
    protects nothing and the scale is ONE draw of the twin's rounding error. Likewise where a tensor has ONE entry that carries the rounding error
    (Tennisbot's action_net.bias and log_std with log_std = (-5, 2): the e^5 of the first component dwarfs the second), device
    error / twin error is the quotient of two draws of one distribution, beyond 24 in 2.7 % of the cases whatever the kernel does.
    The twin is therefore evaluated on ORDERS further orders of the same rows -- each as legitimate a float32 twin -- and the batch
    is taken only if, for every tensor not resting on the floor u max|tensor|, the twin's error in the batch's own order is at least
    half the median of those. Reference only; the scale the GPU test then uses is check_tensors', unchanged."""
    err = lambda t: {k: float(np.abs(np.asarray(t[k], np.float64) - want[k]).max()) for k in want}  # noqa: E731
    own = err(run(rows, np.float32))
    rng = np.random.default_rng(len(rows))
    others = [err(run(rows[rng.permutation(len(rows))], np.float32)) for _ in range(ORDERS)]
    for k in want:
        median = float(np.median([o[k] for o in others]))
        if np.isfinite(median) and median > ref.U32 * float(np.abs(want[k]).max()) and not own[k] >= 0.5 * median:
            return False
    return True


def gpu_batch(key, run, kernel, m, accept=None):
    """(index vector, the rows it selects) of the GPU test of `kernel` at batch m over a fixture's first N_ROWS rows: a repeat and two
    out-of-range entries (edge_fixtures.index_vector); the first of the seeds SEEDS[kernel] + m + 1000 j whose batch is
    `representative`. run(rows, dtype) -> the tensors the test compares; accept(rows): does the batch keep the fixture's regime (all_inactive and
    all_active_outside depend on the batch's mean advantage); key: the fixture's name (the choice is kept)."""
    if (key, kernel, m) not in _cache:
        for j in range(64):
            idx, rows = index_vector(N_ROWS, m, SEEDS[kernel] + m + 1000 * j)
            want = run(rows, np.float64)
            if (accept is None or accept(rows)) and representative(run, rows, want):
                break
        else:
            raise AssertionError("%s %s m = %d: no representative batch among 64 seeds" % (key, kernel, m))
        _cache[key, kernel, m] = (idx, rows, j)
    return _cache[key, kernel, m][:2]


def evaluate(f, kernel, rows, which=None, dtype=np.float64):
    """the tensors the GPU test of `kernel` ('grad', 'fvp', 'search') compares, on `rows` of the fixture, by Mutant(which)"""
    with np.errstate(all="ignore"):
        if kernel == "grad":
            return checked(Mutant(which).loss_and_grads(f.P, *rows_of(f, rows), f.hp, dtype))
        if kernel == "fvp":
            return Mutant(which).fvp(f.P, rows_of(f, rows)[0], fvp_vector(f.P)[1], float(np.float32(tr.CG_DAMPING)), dtype)
        data, x, steps = search_case(f, rows)
        return columns(Mutant(which).search_table(f.P, x, steps.astype(np.float64), *data, dtype))


def all_rows_are(active, results):
    """every row of the float64 run and of the twin `active` (True) or cut off by the clip (False)"""
    return all((r.active == active).all() for r in results)


def gpu_rows(f, kernel, m):
    accept = None
    if f.which in ("all_inactive", "all_active_outside"):
        accept = lambda rows: all_rows_are(f.which == "all_active_outside", [ref.loss_and_grads(f.P, *rows_of(f, rows), f.hp, dt) for dt in (np.float64, np.float32)])  # noqa: E731
    return gpu_batch((f.kname, f.which), lambda rows, dt: evaluate(f, kernel, rows, None, dt), kernel, m, accept)


def batches(f, kernel="grad"):
    """name -> rows of the fixture's first N_ROWS rows: the three prefixes and the three GPU batches"""
    out = {}
    for n in SIZES:
        out["the first %d rows" % n] = np.arange(n)
        out["the GPU %s batch of %d" % (kernel, n)] = gpu_rows(f, kernel, n)[1]
    return out


def rows_of(f, rows):
    return tuple(x[:N_ROWS][rows] for x in f.data)


# ---------------------------------------------------------------------------------------------------------------------- mutants
def _ulp_noise(x, rng):
    """x moved by -1, 0 or +1 float32 ulp at random (x float32, finite or not)"""
    k = rng.integers(-1, 2, x.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(k > 0, np.nextafter(x, np.float32(np.inf)), np.where(k < 0, np.nextafter(x, np.float32(-np.inf)), x))
    return np.where(np.isfinite(x), out, x).astype(np.float32)


class Mutant:
    """ppo_reference.loss_and_grads, trpo_reference.fvp and trpo_reference.search_table with one line changed:
      tanh_ratio_form         tanh(z) = (e - 1) / (e + 1), e = exp(2 z): inf / inf beyond |z| of 44
      stats_float32_one_pass  the advantage's mean and variance from one-pass sums of x and x^2 in `dtype`
      no_adv_epsilon          A_hat = (A - mean) / std, the 1e-8 dropped
      clip_above_only         the clipped term is A_hat min(ratio, 1 + c)
      fvp_inv_std             the FVP's head scaled by exp(-log_std) in place of exp(-2 log_std)
      search_old_sigma        the mean term of the KL divided by the OLD variance
      search_e2_single        the variance term of the KL exp(-dls) in place of exp(-2 dls)
      fast_tanh               no mistake: fast_tanh's formula with +-1 ulp on the exp2 and on the reciprocal (float32 only)
    None: no line changed."""

    def __init__(self, which=None, seed=0):
        self.which, self.rng = which, np.random.default_rng(seed)

    def tanh(self, z):
        if self.which == "tanh_ratio_form":
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(z.dtype.type(2) * z)
                return (e - z.dtype.type(1)) / (e + z.dtype.type(1))
        if self.which == "fast_tanh" and z.dtype == np.float32:
            with np.errstate(over="ignore", under="ignore"):
                e = _ulp_noise(np.exp2((z * np.float32(2.8853900817779268)).astype(np.float64)).astype(np.float32), self.rng)
                r = _ulp_noise((1.0 / (e + np.float32(1.0)).astype(np.float64)).astype(np.float32), self.rng)
            return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)      # one rounding: the kernel's fma
        return np.tanh(z)

    def tower(self, P, body, head, x):
        hs, k = [x], 0
        while "%s.%d.weight" % (body, k) in P:
            hs.append(self.tanh(hs[-1] @ P["%s.%d.weight" % (body, k)].T + P["%s.%d.bias" % (body, k)]))
            k += 2
        return hs, hs[-1] @ P[head + ".weight"].T + P[head + ".bias"]

    def normalise(self, adv, dtype):
        dt = np.dtype(dtype).type
        adv = np.asarray(adv).astype(dtype)
        if self.which == "stats_float32_one_pass":
            B = dt(adv.shape[0])
            sx, sq = adv.sum(dtype=dtype), (adv * adv).sum(dtype=dtype)
            mean = sx / B
            var = (sq - sx * mean) / (B - dt(1))
            return (adv - mean) / (np.sqrt(np.maximum(var, dt(0))) + dt(ref.ADV_EPS))
        if self.which == "no_adv_epsilon":
            with np.errstate(invalid="ignore", divide="ignore"):
                return (adv - adv.mean(dtype=dtype)) / adv.std(ddof=1, dtype=dtype)
        return (adv - adv.mean(dtype=dtype)) / (adv.std(ddof=1, dtype=dtype) + dt(ref.ADV_EPS))

    def loss_and_grads(self, params, obs, act, old_logp, adv, returns, hp, dtype=np.float64):
        dt = np.dtype(dtype).type
        P = ref.cast_params(params, dtype)
        obs, act, old_logp, adv, returns = (np.asarray(x).astype(dtype) for x in (obs, act, old_logp, adv, returns))
        B = adv.shape[0]
        c, vf, ent = dt(hp["clip_range"]), dt(hp["vf_coef"]), dt(hp["ent_coef"])
        a = self.normalise(adv, dtype)
        hs_pi, mean = self.tower(P, "policy_net", "action_net", obs)
        hs_vf, value = self.tower(P, "value_net_body", "value_net", obs)
        value = value[:, 0]
        log_std = P["log_std"]
        inv_std = np.exp(-log_std)
        zeta = (act - mean) * inv_std
        logp = (dt(-0.5) * zeta * zeta - log_std - dt(ref.LN_SQRT_2PI)).sum(-1, dtype=dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            ratio = np.exp(logp - old_logp)
            if self.which == "clip_above_only":
                s1, s2 = a * ratio, a * np.minimum(ratio, dt(1) + c)
            else:
                s1, s2 = a * ratio, a * np.clip(ratio, dt(1) - c, dt(1) + c)
            pg = -np.minimum(s1, s2).mean(dtype=dtype)
            verr = returns - value
            vl = (verr * verr).mean(dtype=dtype)
            entropy = (dt(0.5) + dt(ref.LN_SQRT_2PI) + log_std).sum(dtype=dtype)
            loss = pg + vf * vl - ent * entropy
            active = s1 <= s2
            d_logp = np.where(active, -a * ratio, dt(0)) / dt(B)
            grads = {}
            ref._tower_backward(P, "policy_net", "action_net", hs_pi, (d_logp[:, None] * zeta) * inv_std, grads)
            grads["log_std"] = (d_logp[:, None] * (zeta * zeta - dt(1))).sum(0, dtype=dtype) - ent
            ref._tower_backward(P, "value_net_body", "value_net", hs_vf, (dt(-2) * vf / dt(B) * verr)[:, None], grads)
        stats = {"policy_loss": float(pg), "value_loss": float(vl), "entropy": float(entropy)}
        return ref.Loss(float(loss), grads, stats, ratio, a, active)

    def fvp(self, P, obs, v, damping=tr.CG_DAMPING, dtype=np.float64):
        dt = np.dtype(dtype).type
        Pt, V = ref.cast_params(tr.theta_of(P), dtype), ref.cast_params(tr.theta_of(v), dtype)
        hs, _ = self.tower(Pt, "policy_net", "action_net", np.asarray(obs).astype(dtype))
        m = hs[0].shape[0]
        hd = None
        for i in range(len(hs) - 1):
            W, name = Pt["policy_net.%d.weight" % (2 * i)], "policy_net.%d" % (2 * i)
            zd = hs[i] @ V[name + ".weight"].T + V[name + ".bias"]
            if hd is not None:
                zd = zd + hd @ W.T
            hd = (dt(1) - hs[i + 1] * hs[i + 1]) * zd
        mud = hs[-1] @ V["action_net.weight"].T + V["action_net.bias"] + hd @ Pt["action_net.weight"].T
        if self.which == "fvp_inv_std":
            d_out = mud * np.exp(dt(-1) * Pt["log_std"]) / dt(m)
        else:
            d_out = mud * np.exp(dt(-2) * Pt["log_std"]) / dt(m)
        out = {}
        ref._tower_backward(Pt, "policy_net", "action_net", hs, d_out, out)
        out["log_std"] = dt(2) * V["log_std"]
        return {k: out[k] + dt(damping) * V[k] for k in Pt}

    def search_table(self, P, x, steps, obs, act, old_logp, adv, dtype=np.float64):
        dt = np.dtype(dtype).type
        a = self.normalise(adv, dtype)
        out = np.zeros((len(steps), 2))
        Pc = ref.cast_params(tr.theta_of(P), dtype)
        o = np.asarray(obs).astype(dtype)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for k, s in enumerate(steps):
                P2 = ref.cast_params(tr.theta_of(tr.moved(P, x, s, dtype)), dtype)
                _, mu = self.tower(Pc, "policy_net", "action_net", o)
                _, mu2 = self.tower(P2, "policy_net", "action_net", o)
                ls, ls2 = Pc["log_std"], P2["log_std"]
                zeta = (np.asarray(act).astype(dtype) - mu2) * np.exp(-ls2)
                logp = (dt(-0.5) * zeta * zeta - ls2 - dt(ref.LN_SQRT_2PI)).sum(-1, dtype=dtype)
                ratio = np.exp(logp - np.asarray(old_logp).astype(dtype))
                L = float((ratio * a).mean(dtype=dtype))
                if self.which == "search_old_sigma":
                    m = (ls2 - ls) + dt(0.5) * (np.exp(ls) ** 2 / np.exp(ls2) ** 2 + (mu - mu2) ** 2 / np.exp(ls) ** 2) - dt(0.5)
                elif self.which == "search_e2_single":
                    m = (ls2 - ls) + dt(0.5) * (np.exp(ls) / np.exp(ls2) + (mu - mu2) ** 2 / np.exp(ls2) ** 2) - dt(0.5)
                else:
                    m = (ls2 - ls) + dt(0.5) * (np.exp(ls) ** 2 + (mu - mu2) ** 2) / np.exp(ls2) ** 2 - dt(0.5)
                out[k] = L, float(m.sum(-1, dtype=dtype).mean(dtype=dtype))
        return out


# --------------------------------------------------------------------------------------------------------------------- checking
def ratios(got, want, twin):
    """ppo_reference.tensor_ratios. A tensor that is exactly zero in the float64 reference AND in its twin has no rounding scale:
    it must be exactly zero in `got` (ratio 0), and is infinitely far otherwise."""
    zero = [k for k in want if not np.any(want[k]) and not np.any(twin[k])]
    rest = [k for k in want if k not in zero]
    out = ref.tensor_ratios({k: got[k] for k in rest}, {k: want[k] for k in rest}, {k: twin[k] for k in rest})
    out.update({k: 0.0 if not np.any(got[k]) else np.inf for k in zero})
    return out


def check(name, got, want, twin, multiple=ref.MULTIPLE):
    """ppo_reference.check_tensors over `ratios`"""
    r = ratios(got, want, twin)
    worst = max(r, key=r.get)
    if not r[worst] <= multiple:
        raise AssertionError("%s: %s is %.3g float32-twin errors from the float64 reference (allowed %.3g)" % (name, worst, r[worst], multiple))
    return r[worst]


def checked(res):
    """every tensor the GPU gradient tests hold to the reference, as one dict: the gradients and the three statistics"""
    out = dict(res.grads)
    out.update({k: np.float64(v) for k, v in res.stats.items()})
    return out


def columns(table):
    return {"L": np.asarray(table)[:, 0], "KL": np.asarray(table)[:, 1]}


def finite_rows(table):
    return np.isfinite(np.asarray(table)).all(1)


def fvp_vector(P, seed=8):
    """a float32 vector that is non-zero in every slot, flat and as a dict over theta"""
    n = sum(int(np.size(v)) for v in P.values())
    vec = np.random.default_rng(seed).normal(0.0, 1.0, n).astype(np.float32)
    vec[np.abs(vec) < 1e-3] = 0.5
    return vec, tr.theta_of(tr.split_flat(vec.astype(np.float64), P))


def search_direction(P, data, which, seed=0):
    """(old_logp, direction over theta, steps float32) on the rows of data = (obs, act, old_logp, adv). 'kl': along the surrogate's
    gradient with a first step that leaves the trust region (KL_0 about 3 delta: KL_k = KL_0 1.5^-2k re-enters at k = 2); 'none':
    against the gradient from a behaviour policy that IS theta (L_0 = 0 at a zero step, so every L_k < 0): nothing is accepted;
    'random': a random direction"""
    obs, act, old_logp, adv = data
    theta = tr.theta_of(P)
    if which == "none":
        old_logp = logp64(P, obs, act).astype(np.float32)
    if which == "random":
        rng = np.random.default_rng(seed)
        x = {k: rng.normal(size=np.shape(v)) for k, v in theta.items()}
    else:
        g = tr.surrogate_gradient(P, obs, act, old_logp, adv)
        x = {k: (-v if which == "none" else v) for k, v in g.items()}
    x = {k: v.astype(np.float32).astype(np.float64) for k, v in x.items()}
    probe = 1e-3 / max(np.abs(v).max() for v in x.values())
    c = tr.kl(P, tr.moved(P, x, probe), obs) / probe ** 2                      # KL(s) ~ c s^2
    beta = np.sqrt({"kl": 3.0, "none": 0.5, "random": 1.2}[which] * tr.KL_DELTA / c)
    steps = (beta * tr.DECAY ** -np.arange(tr.CANDIDATES)).astype(np.float32)
    return (obs, act, old_logp, adv), x, steps


def search_fixture(ro, P, rows, which):
    """search_direction on the rollout's own rows (tests/test_gpu_trpo.py)"""
    return search_direction(P, tuple(x[rows] for x in flat_shard(ro, ro.gae.adv, ro.gae.returns)[:4]), which, len(rows))


def nonfinite_step(f, rows, x, steps):
    """the smallest beta 10^j at which the float32 twin's L is no longer finite on `rows`: theta + step x overflows"""
    obs, act, old_logp, adv, _ = rows_of(f, rows)
    for j in range(1, 42):
        s = np.float32(min(float(steps[0]) * 10.0 ** j, 3.0e38))
        if not np.isfinite(Mutant().search_table(f.P, x, [float(s)], obs, act, old_logp, adv, np.float32)[0, 0]):
            return s
    raise AssertionError("no float32 step makes the twin's surrogate non-finite")


def search_case(f, rows, which="kl"):
    """(data, direction, steps) of the line search on `rows` of the fixture. 'overflow_head': the first two steps of 'kl' so large
    that the twin's L_k is not finite, the rest the usual geometric sequence; 'all_nonfinite': every step that large; 'inf_ratio':
    the steps of 'kl' on data whose ratio overflows on one row (inf_ratio_row)"""
    data = rows_of(f, rows)[:4]
    data, x, steps = search_direction(f.P, data, "kl")
    # the direction scaled to a largest network entry of DIRECTION_MAX (the steps shrink by the same factor), so that the largest
    # float32 step carries theta's entries to +-inf. Then the gradient's log_std part rescaled so that the first candidate moves
    # log_std by LOG_STD_MOVE -- left alone it is lost beside the mean's part of the KL, which with log_std = -5 carries a factor
    # of sigma^-2 = e^10 -- and signed so that its largest component SHRINKS sigma: a step of 3e38 sends that log_std to -inf,
    # where zeta = +-inf and logp = -inf + inf, a NaN in either precision
    scale = DIRECTION_MAX / max(np.abs(v).max() for k, v in x.items() if k != "log_std")
    x = {k: f32(v * scale).astype(np.float64) for k, v in x.items()}
    steps = f32(steps.astype(np.float64) / scale)
    ls = x["log_std"] * (LOG_STD_MOVE / (float(steps[0]) * np.abs(x["log_std"]).max()))
    x["log_std"] = f32(-ls if ls[np.argmax(np.abs(ls))] > 0 else ls).astype(np.float64)
    assert np.abs(x["log_std"]).max() >= 2.0
    if which == "inf_ratio":
        obs, act, old_logp, adv = data
        old_logp = old_logp.copy()
        old_logp[rows == inf_ratio_row(f, rows)] = INF_OLD_LOGP
        data = (obs, act, old_logp, adv)
    elif which != "kl":
        big = nonfinite_step(f, rows, x, steps)
        steps = steps.copy()
        steps[:2 if which == "overflow_head" else len(steps)] = big
    return data, x, steps


def inf_ratio_row(f, rows):
    """'inf_ratio': the row of the batch with the largest advantage (A_hat > 0) gets old_logp = INF_OLD_LOGP, so that
    exp(logp - old_logp) is +inf at every ordinary step, in float32 and in float64: L_k = +inf while KL_k is the 'kl' case's, within
    delta from some k on. `L >= 0` and `KL <= delta` both hold there: only the finiteness test of the selection rejects it."""
    return rows[np.argmax(f.data[3][:N_ROWS][rows])]


def mutant_ratio(f, rows, kernel, which):
    """the largest distance, in float32-twin errors, of any tensor the GPU test of `kernel` checks from the float64 reference when
    the float32 evaluation is Mutant(which) on `rows`: (that ratio, its tensor)"""
    r = ratios(evaluate(f, kernel, rows, which, np.float32), evaluate(f, kernel, rows), evaluate(f, kernel, rows, None, np.float32))
    worst = max(r, key=r.get)
    return r[worst], worst


def twin_is_the_references(f, rows):
    """Mutant(None) in float32 and in float64 against the reference modules: the same bits"""
    d = rows_of(f, rows)
    vec, v = fvp_vector(f.P)
    trpo = f.which in WEIGHT_REGIMES            # the FVP and the line search run on the weight regimes only
    if trpo:
        data, x, steps = search_case(f, rows)
    for dt in (np.float64, np.float32):
        a, b = Mutant().loss_and_grads(f.P, *d, f.hp, dt), ref.loss_and_grads(f.P, *d, f.hp, dt)
        same = all(np.array_equal(a.grads[k], b.grads[k]) for k in b.grads) and a.stats == b.stats and a.loss == b.loss and np.array_equal(a.active, b.active)
        if not trpo:
            if not same:
                return False
            continue
        fa, fb = Mutant().fvp(f.P, d[0], v, 1e-3, dt), tr.fvp(f.P, d[0], v, 1e-3, dt)
        same = same and all(np.array_equal(fa[k], fb[k]) for k in fb)
        s64 = steps.astype(np.float64)
        same = same and np.array_equal(Mutant().search_table(f.P, x, s64, *data, dt), tr.search_table(f.P, x, s64, *data, dt))
        if not same:
            return False
    return True


# ------------------------------------------------------------------------------------------------- the tuned net (tb_ppo_grad_net)
TUNED_REGIMES = ("log_std", "all_inactive", "constant_adv", "constant_adv_tenth")
TUNED_CASES = [(name, which) for name in ("sb3", "dead") for which in TUNED_REGIMES] + [("saturating", "saturating")]
TUNED_HEAD = 30.0          # largest |mean| and |value| of the saturating tuned net over its pool


def _tuned_preactivations(P, obs, dtype):
    import tuned_reference as tref
    Pc, o = ref.cast_params(P, dtype), np.asarray(obs).astype(dtype)
    hs, zs = tref._forward(Pc, tref.EXTRACTOR, o)
    return zs + tref._forward(Pc, "policy_net", hs[-1])[1] + tref._forward(Pc, "value_net_body", hs[-1])[1]


def tuned_saturating():
    """The tuned net has no tanh; its counterpart of `saturating` is magnitude. test_tuned_reference.make_policy("saturating"):
    every hidden weight matrix N(0, 2^2), so the hidden pre-activations grow from 1e2 behind the first layer to 4e5 behind the
    last. Left alone the means are of size 1e4 and the ratio's twin error 7.5e-2: no row keeps 100 of those from the clip. So
    both heads are scaled to a largest |output| of TUNED_HEAD over the pool (the means of `sb3` are of that size). 1024
    candidate observations as gradient_fixture draws them; a row is kept if every hidden pre-activation is MARGIN float32-twin
    errors of its own layer (measured on this pool) from 0, so that no float32 forward flips a ReLU.
    (P, pool data, rows that keep the ReLU margin, the layers' twin errors)"""
    import tuned_reference as tref
    from test_tuned_reference import OBS_SCALE, make_policy
    P = {k: v.copy() for k, v in state_dict_arrays(make_policy("saturating", seed=303)).items()}
    rng = np.random.default_rng(303)
    obs = f32(rng.normal(size=(POOL, len(OBS_SCALE))) * OBS_SCALE)
    t = tref.towers(P, obs)
    for head, out in (("action_net", t.mean), ("value_net", t.value)):
        scale = np.float32(TUNED_HEAD / np.abs(out).max())
        for w in (".weight", ".bias"):
            P[head + w] = (P[head + w].astype(np.float32) * scale).astype(np.float64)
    t = tref.towers(P, obs)
    errs = [float(np.abs(b.astype(np.float64) - a).max()) for a, b in zip(_tuned_preactivations(P, obs, np.float64), _tuned_preactivations(P, obs, np.float32))]
    ok = np.all([np.abs(z).min(1) >= MARGIN * e for z, e in zip(_tuned_preactivations(P, obs, np.float64), errs)], 0)
    act = f32(t.mean + np.exp(t.log_std) * rng.normal(size=t.mean.shape))
    zeta = (act - t.mean) * np.exp(-t.log_std)
    old_logp = f32((-0.5 * zeta * zeta - t.log_std - tr.LN_SQRT_2PI).sum(-1) + rng.normal(size=POOL) * 0.15)
    adv, ret = f32(rng.normal(size=POOL) * 2.0 + 0.3), f32(t.value + rng.normal(size=POOL))
    return P, (obs, act, old_logp, adv, ret), ok, errs


def tuned_fixture(name, which):
    """the regime `which` on test_tuned_reference.gradient_fixture(name) (its weights, so its kink margins of the ReLUs stand; only
    log_std, the actions, old_logp or the advantages change), or ("saturating", "saturating"): tuned_saturating().
    (P, hp, data over the kept rows in their order, rows kept, pool). The rows are kept and ordered as in build()."""
    import tuned_reference as tref
    from test_tuned_reference import HP, gradient_fixture
    if ("tuned", name, which) in _cache:
        return _cache["tuned", name, which]
    if which == "saturating":
        P, (obs, act, old_logp, adv, ret), ok, _ = tuned_saturating()
        n = len(adv)
    else:
        fx = gradient_fixture(name)
        P = {k: v.copy() for k, v in state_dict_arrays(fx["policy"]).items()}
        obs, act, old_logp, adv, ret = (fx[k].copy() for k in ("obs", "act", "old_logp", "adv", "returns"))
        n = len(adv)
        ok = np.ones(n, bool)
    rng = np.random.default_rng(9000 + 10 * (TUNED_REGIMES + ("saturating",)).index(which) + len(name))
    t = tref.towers(P, obs)

    def logp(a):
        zeta = (a.astype(np.float64) - t.mean) * np.exp(-P["log_std"])
        return (-0.5 * zeta * zeta - P["log_std"] - tr.LN_SQRT_2PI).sum(-1)

    if which == "log_std":
        P["log_std"] = np.array([-5.0, 2.0])
        act = f32(t.mean + np.exp(P["log_std"]) * rng.normal(size=act.shape))
        old_logp = f32(logp(act) + rng.normal(0.0, 0.15, n))
    elif which == "all_inactive":
        lo, hi = np.quantile(adv, BAND)
        ok &= (adv < lo) | (adv > hi)
        old_logp = f32(logp(act) - np.where(adv > hi, 1.0, -1.0) * rng.uniform(0.3, 1.5, n))
    elif which == "constant_adv":
        adv = np.full(n, 0.25, np.float32)
    elif which == "constant_adv_tenth":
        adv = np.full(n, 0.1, np.float32)
    pool = (obs, act, old_logp, adv, ret)
    want, twin = (tref.loss_and_grads(P, *pool, HP, dt) for dt in (np.float64, np.float32))
    ratio_err = float(np.abs(twin.ratio.astype(np.float64) / want.ratio - 1.0)[ok].max())
    c = HP["clip_range"]
    ok &= np.minimum(np.abs(want.ratio - (1.0 - c)), np.abs(want.ratio - (1.0 + c))) >= MARGIN * ratio_err * want.ratio
    if not which.startswith("constant_adv"):
        ok &= np.abs(want.adv_norm) >= MARGIN * float(np.abs(twin.adv_norm.astype(np.float64) - want.adv_norm).max())
    keep = np.nonzero(ok)[0]
    pos, neg = list(keep[want.adv_norm[keep] > 0]), list(keep[want.adv_norm[keep] <= 0])
    order = []
    while pos and neg:
        order += [pos.pop(0), neg.pop(0)]
    order = np.asarray(order + pos + neg, np.int64)
    out = _cache["tuned", name, which] = (P, dict(HP), tuple(x[order] for x in pool), len(order), n)
    return out


def tuned_rows(name, which, m):
    """gpu_batch for the tuned fixture: the index vector over its first N_ROWS rows"""
    import tuned_reference as tref
    P, hp, data, _, _ = tuned_fixture(name, which)
    run = lambda rows, dt: checked(tref.loss_and_grads(P, *(x[:N_ROWS][rows] for x in data), hp, dt))  # noqa: E731
    accept = None
    if which == "all_inactive":
        accept = lambda rows: all_rows_are(False, [tref.loss_and_grads(P, *(x[:N_ROWS][rows] for x in data), hp, dt) for dt in (np.float64, np.float32)])  # noqa: E731
    return gpu_batch(("tuned", name, which), run, "grad", m, accept)


# ------------------------------------------------------------------------------- the regime left out on purpose (no test)
def tiny_emulation(kname, seeds=4):
    """Hidden pre-activations around 1e-4: first-layer weights N(0, 1e-5^2), later hidden weights N(0, 1 / fan_in), hidden biases
    N(0, 1e-4^2) in both towers (generator seed 5), make_policy's heads, on the first N_ROWS rows of the `saturating` fixture's data
    as ONE batch. Per tensor the largest distance, over `seeds` noise seeds, of the emulated fast_tanh twin from the float64
    reference in float32-twin errors: fast_tanh's error is absolute, np.tanh's relative, and a weight gradient is d_out^T h."""
    f = build(kname, "saturating")
    P = {k: v.copy() for k, v in build(kname, "offset_adv").P.items()}          # make_policy's weights
    rng = np.random.default_rng(5)
    for k in P:
        if k.startswith(("policy_net.", "value_net_body.")):
            std = 1e-4 if k.endswith(".bias") else 1e-5 if k.split(".")[1] == "0" else P[k].shape[1] ** -0.5
            P[k] = f32(rng.normal(0.0, std, P[k].shape)).astype(np.float64)
    data = tuple(x[:N_ROWS] for x in f.data)
    want, twin = (checked(Mutant().loss_and_grads(P, *data, f.hp, dt)) for dt in (np.float64, np.float32))
    worst = {}
    for seed in range(seeds):
        r = ratios(checked(Mutant("fast_tanh", seed).loss_and_grads(P, *data, f.hp, np.float32)), want, twin)
        worst = {k: max(worst.get(k, 0.0), v) for k, v in r.items()}
    return worst
