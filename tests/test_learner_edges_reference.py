"""The on-policy learner kernels' edge fixtures (tests/learner_edge_fixtures.py) on CPU: every fixture of both env kinds keeps the
conditions it was built for -- on the first 17, 129 and 257 kept rows, on the batches the GPU tests draw from them and on rows 0
and 256, which every such batch holds --, the float32 twin takes the same side of the clip on every kept row, the unmutated
`Mutant` is the reference's own twin bit for bit, and each of the seven one-line mutants lies more than ppo_reference.MULTIPLE twin
errors from the float64 reference on the fixture named for it, at every size. Nothing here runs a kernel.

The one exemption: with every advantage float32(0.1) (constant_adv_tenth) A_hat is exactly 0 in float64 and on the device (sums
of 257 equal 24-bit numbers are exact in float64), while the float32 TWIN's mean of 257 such numbers is not 0.1 and its A_hat is a
number of size 0.4: the twin is no scale there, its `active` is not compared, and the GPU test asserts the derived exact values.

The smallest rejection ratio per mutant and the twin error per fixture are printed, and quoted in DESIGN.md."""
import numpy as np
import pytest

import learner_edge_fixtures as lf
import ppo_reference as ref
import trpo_reference as tr

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("learner edges (cpu): %s = %.3g" % (k, WORST[k]))


def results(f, rows):
    return tuple(ref.loss_and_grads(f.P, *lf.rows_of(f, rows), f.hp, dt) for dt in (np.float64, np.float32))


@pytest.mark.parametrize("which", lf.REGIMES)
@pytest.mark.parametrize("kname", list(lf.CASE))
def test_fixture_keeps_its_conditions(kname, which):
    f = lf.build(kname, which)
    tag = "%s %s" % (kname, which)
    c = f.hp["clip_range"]
    assert f.kept >= lf.POOL // 2 and len(f.keep) == f.kept >= lf.N_ROWS, "%s: %d of %d rows kept" % (tag, f.kept, lf.POOL)
    assert len(set(f.keep)) == len(f.keep)
    obs, act, old_logp, adv, ret = (x[:lf.N_ROWS] for x in f.data)
    # per row, on a fresh evaluation of the first N_ROWS rows (rows 0 and N_ROWS - 1 among them, named because every GPU batch holds them)
    want, twin = results(f, np.arange(lf.N_ROWS))
    log_ratio = lf.logp64(f.P, obs, act) - old_logp
    ratio = np.exp(log_ratio)
    edge = np.minimum(np.abs(ratio - (1.0 - c)), np.abs(ratio - (1.0 + c)))
    assert (edge >= lf.MARGIN * f.ratio_err * ratio).all()
    if not f.constant:      # the pool-normalised A_hat of the kept rows, as the rejection measured it
        assert (np.abs(f.pool_adv_norm[f.keep[:lf.N_ROWS]]) >= lf.MARGIN * f.adv_err).all()
    for n in lf.SIZES + (1,):       # ... which is every condition of a row: it holds for each prefix and for rows 0 and N_ROWS - 1 alone
        sel = np.arange(n) if n > 1 else np.array([0, lf.N_ROWS - 1])
        assert (edge[sel] >= lf.MARGIN * f.ratio_err * ratio[sel]).all() and (f.constant or (np.abs(f.pool_adv_norm[f.keep[sel]]) >= lf.MARGIN * f.adv_err).all())
    outside = (ratio < 1.0 - c) | (ratio > 1.0 + c)
    for body in ("policy_net", "value_net_body"):
        hs, z0 = lf.hidden(f.P, obs, body, "action_net" if body == "policy_net" else "value_net")
        if which == "overflow":
            assert z0[:, 0].min() >= lf.OVERFLOW_Z and z0[:, 1].max() <= -lf.OVERFLOW_Z 
            assert (hs[0][:, 0] == 1.0).all() and (hs[0][:, 1] == -1.0).all()       # exactly +-1 in float64 already
    if which == "saturating":
        for n in lf.SIZES:
            share = lf.saturated_share(f.P, obs[:n])
            assert share >= 0.5, "%s: %.3f of the hidden activations of the first %d rows beyond %.3f" % (tag, share, n, lf.SATURATED)
        assert min(lf.saturated_share(f.P, obs[i:i + 1]) for i in (0, lf.N_ROWS - 1)) >= 0.5
        print("%s: %.3f of all hidden activations have |h| > %.3f" % (tag, lf.saturated_share(f.P, obs), lf.SATURATED))
    if which == "log_std":
        assert np.array_equal(f.P["log_std"], np.resize([-5.0, 2.0], f.A))
    if which in ("all_inactive", "all_active_outside"):
        assert outside.all()
    if which == "wide_ratio":
        assert log_ratio.min() < -15.0 and log_ratio.max() > 15.0 and np.abs(log_ratio).max() < 21.0 and all(np.abs(log_ratio[:n]).max() > 10.0 for n in lf.SIZES)
    if which == "constant_adv":
        assert (adv == np.float32(0.25)).all()
    if which == "constant_adv_tenth":
        assert (adv == np.float32(0.1)).all()
    if which == "offset_adv":
        assert np.abs(adv - lf.OFFSET).max() < 5.0 * lf.OFFSET_SCALE and adv.std() > 0.5 * lf.OFFSET_SCALE
    # per batch: the three prefixes and the three batches the GPU gradient test draws
    for name, rows in lf.batches(f).items():
        assert 0 in rows and (lf.N_ROWS - 1 in rows or name.startswith("the first"))
        w, t = results(f, rows)
        if which != "constant_adv_tenth":
            assert np.array_equal(w.active, t.active), "%s, %s: the float32 twin took another side of the clip" % (tag, name)
        if not f.constant:
            # (the margin of |A_hat| is the pool's, as the rejection's; inside a batch the mean is another one: the sign is what it protects)
            assert np.array_equal(w.adv_norm > 0, t.adv_norm > 0) and w.adv_norm.all(), "%s, %s: the float32 twin's A_hat has another sign" % (tag, name)
        else:
            assert not w.adv_norm.any() and w.stats["policy_loss"] == 0.0
            assert not any(np.any(v) for k, v in w.grads.items() if tr.is_theta(k) and k != "log_std") and (w.grads["log_std"] == -f.hp["ent_coef"]).all()
        if which == "all_inactive":
            assert not w.active.any() and not t.active.any(), "%s, %s: an active row" % (tag, name)
            assert not any(np.any(v) for k, v in w.grads.items() if tr.is_theta(k) and k != "log_std") and (w.grads["log_std"] == -f.hp["ent_coef"]).all()
        if which == "all_active_outside":
            assert w.active.all() and t.active.all(), "%s, %s: an inactive row" % (tag, name)
            free = ref.loss_and_grads(f.P, *lf.rows_of(f, rows), dict(f.hp, clip_range=np.inf))
            assert all(np.array_equal(free.grads[k], w.grads[k]) for k in w.grads) and free.stats == w.stats
        if which in lf.WEIGHT_REGIMES + ("wide_ratio", "offset_adv"):
            assert 0.0 < w.active.mean() and (which != "wide_ratio" or w.active.mean() < 1.0)
    assert lf.twin_is_the_references(f, np.arange(lf.SIZES[0])) and lf.twin_is_the_references(f, lf.gpu_rows(f, "grad", lf.SIZES[1])[1])
    # the twin's own error on what the GPU tests compare, and the emulated twin's (fast_tanh's formula, +-1 ulp on exp2 and rcp)
    scale = ref.twin_scale(lf.checked(want), lf.checked(twin))
    names = list(want.grads)
    g_err, g_size = max(scale[k] for k in names), max(np.abs(want.grads[k]).max() for k in names)
    emu = max(lf.mutant_ratio(f, rows, "grad", "fast_tanh")[0] for rows in lf.batches(f).values()) if which != "constant_adv_tenth" else float("nan")
    print("%s: %d of %d rows kept; twin error: ratio %.3g relative, A_hat %.3g, gradients %.3g (largest entry %.3g); emulated fast_tanh twin %.3g twin errors"
          % (tag, f.kept, lf.POOL, f.ratio_err, f.adv_err, g_err, g_size, emu))
    WORST["emulated gradient, largest, %s" % which] = max(WORST.get("emulated gradient, largest, %s" % which, 0.0), emu)


@pytest.mark.parametrize("which", lf.WEIGHT_REGIMES)
@pytest.mark.parametrize("kname", list(lf.CASE))
def test_fvp_and_search_fixtures(kname, which):
    f = lf.build(kname, which)
    tag = "%s %s" % (kname, which)
    vec, v = lf.fvp_vector(f.P)
    assert np.all(vec != 0.0)
    for kernel in ("fvp", "search"):
        emu = max(lf.mutant_ratio(f, rows, kernel, "fast_tanh")[0] for rows in lf.batches(f, kernel).values())
        assert max(lf.mutant_ratio(f, rows, kernel, None)[0] for rows in lf.batches(f, kernel).values()) <= 1.0
        print("%s: emulated fast_tanh twin of the %s: %.3g twin errors" % (tag, kernel, emu))
        WORST["emulated %s, largest, %s" % (kernel, which)] = max(WORST.get("emulated %s, largest, %s" % (kernel, which), 0.0), emu)
    for name, rows in lf.batches(f, "search").items():
        picked = {}
        for case in ("kl", "overflow_head", "all_nonfinite"):
            data, x, steps = lf.search_case(f, rows, case)
            assert np.all(x["log_std"] != 0.0) and len(steps) == tr.CANDIDATES
            s64 = steps.astype(np.float64)
            with np.errstate(all="ignore"):            # the giant steps overflow on purpose
                want, twin = tr.search_table(f.P, x, s64, *data), tr.search_table(f.P, x, s64, *data, np.float32)
            fin = lf.finite_rows(twin)
            assert np.array_equal(fin, lf.finite_rows(want)) or case != "kl"
            head = {"kl": 0, "overflow_head": 2, "all_nonfinite": tr.CANDIDATES}[case]
            assert not np.isfinite(twin[:head, 0]).any() and fin[head:].all(), "%s, %s, %s: finite candidates %s" % (tag, name, case, fin)
            if fin.any():
                margins = tr.threshold_margins(want[fin], twin[fin])
                assert margins.min() > lf.MARGIN, "%s, %s, %s: a candidate sits %.3g twin errors from its threshold" % (tag, name, case, margins.min())
            picked[case] = tr.select(want)
            assert picked[case] == tr.select(twin)
        data, x, steps = lf.search_case(f, rows, "inf_ratio")
        with np.errstate(all="ignore"):
            want, twin = tr.search_table(f.P, x, steps.astype(np.float64), *data), tr.search_table(f.P, x, steps.astype(np.float64), *data, np.float32)
        # +inf beside a KL within delta: `L >= 0 and KL <= delta` alone would accept it
        assert (want[:, 0] == np.inf).all() and (twin[:, 0] == np.inf).all() and np.isfinite(twin[:, 1]).all() and (twin[:, 1] <= tr.KL_DELTA).any()
        assert tr.select(want) == tr.select(twin) == -1 and (data[2] == lf.INF_OLD_LOGP).sum() >= 1
        assert picked["all_nonfinite"] == -1 and picked["overflow_head"] in (-1,) + tuple(range(2, tr.CANDIDATES))
        if picked["kl"] >= 2:
            assert picked["overflow_head"] == picked["kl"]          # the later candidates are the same steps


@pytest.mark.parametrize("which", list(lf.MUTANTS))
@pytest.mark.parametrize("kname", list(lf.CASE))
def test_mutant_is_rejected_by_its_fixture(kname, which):
    regime, kernel = lf.MUTANTS[which]
    f = lf.build(kname, regime)
    worst = np.inf
    for name, rows in lf.batches(f, kernel).items():
        assert lf.mutant_ratio(f, rows, kernel, None)[0] <= 1.0                 # no line changed: the twin itself passes
        r, tensor = lf.mutant_ratio(f, rows, kernel, which)
        assert r > ref.MULTIPLE, "%s %s: the mutant %s is %.3g twin errors away on %s (%s): it would pass" % (kname, regime, which, r, name, tensor)
        worst = min(worst, r)
    print("%s %s: mutant %s: at least %.3g twin errors from the reference" % (kname, regime, which, worst))
    WORST["mutant %s, smallest rejection ratio" % which] = min(WORST.get("mutant %s, smallest rejection ratio" % which, np.inf), worst)


def test_a_lucky_twin_is_not_representative():
    """a one-entry tensor whose twin, in the batch's own order, lands 100 times nearer the reference than in every other order"""
    want, rows = {"b": np.array([1e-4])}, np.arange(17)

    def run(r, dtype, lucky=1e-11):
        return {"b": want["b"] + (lucky if np.array_equal(r, rows) else 1e-9)}

    assert not lf.representative(run, rows, want)
    assert lf.representative(lambda r, dt: run(r, dt, 0.7e-9), rows, want)
    assert lf.representative(lambda r, dt: {"b": want["b"] * (1.0 + 1e-9)}, rows, want)        # at the floor u |tensor|: the floor is the scale


def test_index_vector_is_the_gpu_modules():
    """the batches above are the ones the GPU modules draw: one index_vector and one choice of seed for all of them"""
    import edge_fixtures
    assert lf.index_vector is edge_fixtures.index_vector
    f = lf.build("swing", "overflow")
    for kernel in lf.SEEDS:
        for m in lf.SIZES:
            idx, rows = lf.gpu_rows(f, kernel, m)
            assert len(idx) == m and idx[0] == idx[m - 1] and idx[1] < 0 and idx[m // 2] >= lf.N_ROWS and rows[1] == 0 and rows[m // 2] == lf.N_ROWS - 1
            assert lf.gpu_rows(f, kernel, m)[0] is idx


@pytest.mark.parametrize("name,which", lf.TUNED_CASES)
def test_tuned_fixture_keeps_its_conditions(name, which):
    import tuned_reference as tref
    P, hp, data, kept, pool = lf.tuned_fixture(name, which)
    assert kept >= max(lf.N_ROWS, pool // 2), "%d of %d rows kept" % (kept, pool)
    data = tuple(x[:lf.N_ROWS] for x in data)
    pre = tref.towers(P, data[0]).pre
    assert min(float(np.abs(z).min()) for z in pre) >= tref.KINK_MARGIN      # the ReLUs' margin stands
    if which == "saturating":
        _, _, _, errs = lf.tuned_saturating()
        z64, z32 = lf._tuned_preactivations(P, data[0], np.float64), lf._tuned_preactivations(P, data[0], np.float32)
        for z, e, a, b in zip(pre, errs, z64, z32):
            assert np.abs(z).min() >= lf.MARGIN * e and np.array_equal(a > 0, b > 0)      # its own: 100 twin errors per layer, no ReLU flipped
        t = tref.towers(P, data[0])
        assert max(np.abs(z).max() for z in pre) > 1e5 and 10.0 < np.abs(t.mean).max() <= 1.01 * lf.TUNED_HEAD
        print("tuned saturating: %d of %d rows kept; largest pre-activation per layer %s, its twin error %s"
              % (kept, pool, " ".join("%.3g" % np.abs(z).max() for z in pre), " ".join("%.3g" % e for e in errs)))
    for name_, rows in [("the first %d rows" % n, np.arange(n)) for n in lf.SIZES] + [("the GPU batch of %d" % n, lf.tuned_rows(name, which, n)[1]) for n in lf.SIZES]:
        batch = tuple(x[rows] for x in data)
        w, t = tref.loss_and_grads(P, *batch, hp), tref.loss_and_grads(P, *batch, hp, np.float32)
        if which != "constant_adv_tenth":
            assert np.array_equal(w.active, t.active), name_
        if which == "all_inactive":
            assert not w.active.any() and not any(np.any(v) for k, v in w.grads.items() if tr.is_theta(k) and k != "log_std")
        if which.startswith("constant_adv"):
            assert not w.adv_norm.any() and w.stats["policy_loss"] == 0.0
        if which in ("log_std", "saturating"):
            assert 0.0 < w.active.mean()
        if which == "log_std":
            assert np.array_equal(P["log_std"], [-5.0, 2.0])
