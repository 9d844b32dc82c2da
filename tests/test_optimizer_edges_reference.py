"""The optimizer edge fixtures (tests/optimizer_edge_fixtures.py) on CPU. Nothing here runs a kernel.

  * the step counts and clip bounds are the computed ones, and the vectors keep the conditions they are built for;
  * on the ordinary classes the restated step is within ppo_reference.MULTIPLE float32-twin errors of ppo_reference's
    clip_global_norm + adam_step in float64 (the twin: the same pair in float32; the betas are the float32 values), and so is torch
    on the CPU in float32 (clip_grad_norm_, then torch.optim.Adam with the moments and the step count written into its state), at
    every step of steps(), world 1 and 3 and every bound;
  * on the four non-finite gradients the restatement's NaN / inf / unchanged-bits pattern per slot of p, g, m and v is torch's;
  * each one-line mutant is rejected by the bit comparison the GPU test makes, on the case named for it in MUTANT_CASES.

ONE MUTANT'S CASE IS NOT THE ONE FIRST NAMED FOR IT. c2_powf (c2 = 1.0f - powf(beta2, step)) was to be rejected at a step near the
edge where c2 becomes 1.0f. It cannot be: there x = beta2^step is about 2^-25, powf's error in x is about 2^-49, and 1 - x is
rounded to a grid of 2^-24, so both routes round to the same float (a difference needs a rounding boundary of 1 - x inside an
interval 2^-25 times as wide as the grid). The routes part where 1 - x cancels: at step 2, x = 0.998, 1.0f - x is exact in float32
and carries powf's rounding of x, 2^-24, into a c2 of 0.002 whose own grid is 2^-33. test_mutant_is_rejected takes step 2 and
asserts beside it that the two routes give the same c2 at both edge steps, so the claim stays checked.
"""
import numpy as np
import pytest

import optimizer_edge_fixtures as fx
import ppo_reference as ref

F = fx.F
HP = dict(lr=fx.LR, beta1=fx.BETA1, beta2=fx.BETA2, eps=fx.ADAM_EPS)
BETAS32 = (float(F(fx.BETA1)), float(F(fx.BETA2)))
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("optimizer edges (cpu): %s = %.3g" % (k, WORST[k]))


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)


def tensors(p0, out, lr=fx.LR):
    p, g, m, v = out
    return {"param_change": (np.asarray(p, np.float64) - np.asarray(p0, np.float64)) / lr, "grad": g, "exp_avg": m, "exp_avg_sq": v}


def reference_step(p, g, m, v, world, max_norm, step, dtype):
    """ppo_reference: the gradient averaged over the ranks, clipped, Adam"""
    dt = np.dtype(dtype).type
    grads = {"x": g.astype(dtype) / dt(world) if world > 1 else g.astype(dtype)}
    clipped, _ = ref.clip_global_norm(grads, float(max_norm), dtype)
    state = {"t": step - 1, "m": {"x": m.astype(dtype)}, "v": {"x": v.astype(dtype)}}
    with np.errstate(over="ignore", invalid="ignore"):
        new = ref.adam_step({"x": p.astype(dtype)}, clipped, state, fx.LR, betas=BETAS32, eps=fx.ADAM_EPS, dtype=dtype)
    return new["x"], clipped["x"], state["m"]["x"], state["v"]["x"]


def torch_step(torch, p, g, m, v, world, max_norm, step):
    """torch on the CPU in float32: clip_grad_norm_ then Adam(eps=1e-5).step() from the given moments and step count"""
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy((g / F(world) if world > 1 else g).copy())
    torch.nn.utils.clip_grad_norm_([tp], float(max_norm))
    opt = torch.optim.Adam([tp], lr=fx.LR, betas=BETAS32, eps=fx.ADAM_EPS)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.step()
    st = opt.state[tp]
    return tuple(x.detach().numpy().copy() for x in (tp, tp.grad, st["exp_avg"], st["exp_avg_sq"]))


# ------------------------------------------------------------------------------------------------------------ the fixtures themselves
def test_steps_are_the_computed_edges():
    e1, e2 = fx.step_edges()
    steps = fx.steps()
    c = {s: fx.bias_corrections(fx.BETA1, fx.BETA2, s) for s in steps}
    assert c[e1 - 1][0] < 1 and c[e1][0] == 1 and c[e2 - 1][1] < 1 and c[e2][1] == 1
    assert c[e1 - 1][0] == fx.BELOW_ONE and c[e2 - 1][1] == fx.BELOW_ONE        # the last float32 below 1: the edge, not a step near it
    assert steps == sorted(steps) and steps[:2] == [1, 2] and 1000 in steps and 10 ** 6 in steps and steps[-1] == 3 * 10 ** 9 and len(steps) == 9
    assert all(c[s][0] == 1 and c[s][1] == 1 for s in steps if s >= e2) and all(0 < c[s][1] < 1 for s in steps if s < e2)
    print("c1 is 1.0f from step %d on, c2 from step %d on; steps() = %s" % (e1, e2, steps))


@pytest.mark.parametrize("name", list(fx.NETS))
def test_vectors_keep_their_conditions(name):
    L = fx.Layout(name)
    for with_extremes in (False, True):
        p, g, m, v, classes = fx.vectors(L.P, 3, with_extremes)
        kinds = fx.CLASSES if with_extremes else fx.ORDINARY
        assert set(classes) == set(kinds)
        assert np.isin(classes, fx.EXTREME).sum() * 4 <= L.P
        regions = [(0, fx.LANES), (fx.LANES, L.P)] + (list(L.critic) + list(L.policy) if L.critic else [])
        for lo, hi in regions:
            assert set(classes[lo:hi]) == set(kinds), (lo, hi)
        is_ = {c: classes == c for c in kinds}
        a = np.abs(g)
        assert (a[is_["ordinary"]] >= F(1e-6)).all() and (a[is_["ordinary"]] <= 1).all()
        assert not g[is_["zero_g"]].any() and m[is_["zero_g"]].all() and v[is_["zero_g"]].all()
        assert not (g[is_["all_zero"]].any() or m[is_["all_zero"]].any() or v[is_["all_zero"]].any())
        assert (np.sign(m[is_["opposed"]]) == -np.sign(g[is_["opposed"]])).all() and g[is_["opposed"]].all()
        if with_extremes:
            assert (a[is_["tiny"]] >= F(1e-23)).all() and (a[is_["tiny"]] <= F(1e-19)).all()
            assert (a[is_["huge"]] >= F(1e18)).all() and (a[is_["huge"]] <= F(1.8e19)).all()
            assert (a[is_["overflow"]] == F(3e19)).all() and np.isfinite(v[is_["overflow"]]).all() and np.isinf(v[is_["stale_inf"]]).all()
            for step in fx.steps():
                out = fx.step_restated(p, g, m, v, world=1, max_norm=np.inf, step=step, ranges=L.everything, **HP)
                fx.class_invariants(classes, (p, g, m, v), out, step)
                assert np.array_equal(fx.bits(out[1]), fx.bits(g))          # a factor of exactly 1 leaves the gradient's bits
                pa, ma, va = fx.adam_restated(p, g, m, v, step=step, **HP)     # without a clip the two kernels are one formula
                assert all(fx.same_bits(x, y) for x, y in zip((pa, ma, va), (out[0], out[2], out[3])))


@pytest.mark.parametrize("name", list(fx.NETS))
def test_clip_bounds_give_their_factors(name):
    L = fx.Layout(name)
    for ranges in (L.everything,) + ((L.critic,) if L.critic else ()):
        for world in (1, 2, 3):
            seed, (p, g, m, v, _), bounds = fx.sharpest_case(L.P, world, ranges)
            assert seed < fx.MAX_SEEDS and list(bounds) == list(fx.BOUNDS)
            mask = fx.mask_of(L.P, ranges)
            for which, b in bounds.items():
                out = fx.step_restated(p, g, m, v, world=world, max_norm=b, step=7, ranges=ranges, **HP)
                gw = g / F(world) if world > 1 else g
                if which in ("exact_one", "just_misses", "inf"):
                    assert np.array_equal(fx.bits(out[1])[mask], fx.bits(gw)[mask])
                else:
                    moved = mask & (gw != 0)                                             # (zero gradients keep their bits under any factor)
                    assert (fx.bits(out[1])[moved] != fx.bits(gw)[moved]).mean() > 0.99
                assert all(np.array_equal(fx.bits(o)[~mask], fx.bits(i)[~mask]) for o, i in zip(out, (p, g, m, v)))
            print("%s, %s, world %d: seed %d, bounds %s" % (name, "every slot" if ranges is L.everything else "the critic's slots", world, seed,
                                                            ", ".join("%s %.9g" % (k, b) for k, b in bounds.items())))


# ------------------------------------------------------------------------------------------------- float64 and torch comparisons
@pytest.mark.parametrize("world", (1, 3))
@pytest.mark.parametrize("name", list(fx.NETS))
def test_restated_step_is_the_float64_reference_and_torch(name, world):
    import torch
    L = fx.Layout(name)
    _, (p, g, m, v, _), bounds = fx.finite_case(L.P, world, L.everything)
    for step in fx.steps():
        for which, b in bounds.items():
            tag = "%s world %d step %d %s" % (name, world, step, which)
            got = fx.step_restated(p, g, m, v, world=world, max_norm=b, step=step, ranges=L.everything, **HP)
            want, twin = (tensors(p, reference_step(p, g, m, v, world, b, step, dt)) for dt in (np.float64, np.float32))
            note("restated step / twin error", ref.check_tensors(tag, tensors(p, got), want, twin, ref.MULTIPLE))
            note("torch step / twin error", ref.check_tensors(tag + " (torch)", tensors(p, torch_step(torch, p, g, m, v, world, b, step)), want, twin, ref.MULTIPLE))


def test_restated_adam_and_polyak_are_the_float64_formulas():
    n = 1025
    p, g, m, v, _ = fx.vectors(n, 11)
    for step in fx.steps():
        got = fx.adam_restated(p, g, m, v, step=step, **HP)
        want, twin = (reference_step(p, g, m, v, 1, np.inf, step, dt) for dt in (np.float64, np.float32))
        pick = lambda o: {"param_change": (np.asarray(o[0], np.float64) - p) / fx.LR, "exp_avg": o[-2], "exp_avg_sq": o[-1]}  # noqa: E731
        note("restated Adam / twin error", ref.check_tensors("adam step %d" % step, pick(got), pick(want), pick(twin), ref.MULTIPLE))
    # Polyak: each product within u = 2^-24 of itself (half an ulp), the sum within u of itself: 2 u (|omt t| + |tau p|) to first order
    t = np.random.default_rng(5).normal(0.0, 1.0, n).astype(F)
    for tau in (0.005, 0.37, 1.0, 0.0):
        got = fx.polyak_restated(p, t, tau).astype(np.float64)
        omt, tf = float(F(1.0 - float(F(tau)))), float(F(tau))        # the two float32 factors the kernel is handed
        exact = omt * t.astype(np.float64) + tf * p.astype(np.float64)
        assert (np.abs(got - exact) <= 2.0 * 2.0 ** -24 * (1.0 + 2.0 ** -20) * (np.abs(omt * t) + np.abs(tf * p)) + 2.0 ** -148).all(), tau
    assert np.array_equal(fx.bits(fx.polyak_restated(p, t, 0.0)), fx.bits(t)) and np.array_equal(fx.bits(fx.polyak_restated(p, t, 1.0)), fx.bits(p))


# ---------------------------------------------------------------------------------------------------------- non-finite gradients
EXPECTED_NAN = {"nan_slot": "every", "inf_slot_inf_bound": "every", "norm_overflows": "every", "inf_slot": "one"}


@pytest.mark.parametrize("case", fx.NONFINITE_CASES)
@pytest.mark.parametrize("name", ("swing-default", "tennis-tuned"))
def test_nonfinite_gradients_leave_torchs_pattern(name, case):
    import torch
    L = fx.Layout(name)
    p, g0, m, v, _ = fx.vectors(L.P, 21)
    g, max_norm = fx.nonfinite_case(case, g0, L.everything)
    got = fx.step_restated(p, g, m, v, world=1, max_norm=max_norm, step=7, ranges=L.everything, **HP)
    want = torch_step(torch, p, g, m, v, 1, max_norm, 7)
    for what, before, a, b in zip(("params", "grad", "exp_avg", "exp_avg_sq"), (p, g, m, v), got, want):
        pa, pb = fx.pattern(before, a), fx.pattern(before, b)
        assert np.array_equal(pa, pb), "%s %s: %s differs from torch's pattern in %d slots" % (name, case, what, int((pa != pb).sum()))
        nan = int((pa == fx.NAN).sum())
        assert nan == (L.P if EXPECTED_NAN[case] == "every" else 1), (what, nan)
    if case == "inf_slot":      # a factor of 0: every other gradient is (signed) zero, as torch's [0, nan, 0, 0]
        assert int((got[1] == 0).sum()) == L.P - 1
    # the rule before the fix: the NaN is dropped, and only the planted slot (or none) differs from a finite step
    old = fx.Mutant("fminf_clip").step(p, g, m, v, world=1, max_norm=max_norm, step=7, ranges=L.everything, **HP)
    if EXPECTED_NAN[case] == "every":
        assert not np.array_equal(fx.pattern(p, old[0]), fx.pattern(p, want[0])) and int(np.isnan(old[0]).sum()) <= 1
    # the reference helper keeps the NaN too, in both precisions
    # (3e38 squared overflows float32 alone: in float64 that norm is finite and the factor 1)
    for dt in (np.float32,) if case == "norm_overflows" else (np.float64, np.float32):
        clipped, _ = ref.clip_global_norm({"x": g}, float(max_norm), dt)
        assert np.array_equal(np.isnan(clipped["x"]), np.isnan(got[1])), dt


def test_reference_clip_is_unchanged_on_finite_norms():
    rng = np.random.default_rng(2)
    G = {"a": rng.normal(0, 1, (7, 5)), "b": rng.normal(0, 1, 9)}
    for dt in (np.float64, np.float32):
        d = np.dtype(dt).type
        for max_norm in (0.5, 100.0, np.inf):
            clipped, norm = ref.clip_global_norm(G, max_norm, dt)
            n = d(np.sqrt(sum((x.astype(dt) ** 2).sum(dtype=dt) for x in G.values()), dtype=dt))
            coef = min(d(1.0), d(max_norm) / (n + d(ref.NORM_EPS)))           # the rule as it was, which is the same on a finite norm
            assert norm == float(n) and all(np.array_equal(clipped[k], G[k].astype(dt) * d(coef)) for k in G)


# ------------------------------------------------------------------------------------------------------------------- the mutants
def differs(a, b, slots):
    """the GPU test's comparison would fail: some array of `a` is not `b` bit for bit on `slots`"""
    return any(not fx.same_bits(np.asarray(x)[slots], np.asarray(y)[slots]) for x, y in zip(a, b))


MUTANT_CASES = {"c2_powf": "step 2 (see the module docstring)", "v_association": "the ordinary class", "rsqrt_form": "the zero_g class", "fminf_clip": "the NaN slot",
                "norm_float32": "the just_below bound", "polyak_fma": "ordinary slots", "world_after_clip": "world = 3"}


@pytest.mark.parametrize("which", fx.MUTANTS)
def test_mutant_is_rejected(which):
    assert set(MUTANT_CASES) == set(fx.MUTANTS)
    L = fx.Layout("swing-mlp64")
    every = L.everything
    mut, plain = fx.Mutant(which), fx.Mutant()
    _, (p, g, m, v, classes), bounds = fx.finite_case(L.P, 1, every)
    kw = dict(world=1, max_norm=bounds["inf"], step=7, ranges=every, **HP)
    all_slots = np.ones(L.P, bool)
    if which == "c2_powf":
        e2 = fx.step_edges()[1]
        assert all(mut.corrections(fx.BETA1, fx.BETA2, s) == plain.corrections(fx.BETA1, fx.BETA2, s) for s in (e2 - 1, e2))
        kw["step"] = 2
        assert mut.corrections(fx.BETA1, fx.BETA2, 2)[1] != plain.corrections(fx.BETA1, fx.BETA2, 2)[1]
        assert differs(mut.step(p, g, m, v, **kw), plain.step(p, g, m, v, **kw), classes == "ordinary")
        assert differs(mut.adam(p, g, m, v, step=2, **HP), plain.adam(p, g, m, v, step=2, **HP), classes == "ordinary")
    elif which in ("v_association", "rsqrt_form"):
        slots = classes == ("ordinary" if which == "v_association" else "zero_g")
        for step in fx.steps():
            kw["step"] = step
            assert differs(mut.step(p, g, m, v, **kw), plain.step(p, g, m, v, **kw), slots), step
            assert differs(mut.adam(p, g, m, v, step=step, **HP), plain.adam(p, g, m, v, step=step, **HP), slots), step
    elif which == "fminf_clip":
        gn, b = fx.nonfinite_case("nan_slot", g, every)
        kw["max_norm"] = b
        assert differs(mut.step(p, gn, m, v, **kw), plain.step(p, gn, m, v, **kw), all_slots)
        assert not differs(mut.step(p, g, m, v, **kw), plain.step(p, g, m, v, **kw), all_slots)        # ... and by nothing else
    elif which == "norm_float32":
        _, (p, g, m, v, classes), bounds = fx.finite_case(L.P, 1, every, strict=True)
        kw["max_norm"] = bounds["just_below"]
        assert differs(mut.step(p, g, m, v, **kw), plain.step(p, g, m, v, **kw), classes == "ordinary")
    elif which == "polyak_fma":
        t = np.random.default_rng(5).normal(0.0, 1.0, L.P).astype(F)
        for tau in (0.005, 0.37):
            assert differs([mut.polyak(p, t, tau)], [plain.polyak(p, t, tau)], classes == "ordinary"), tau
    else:
        _, (p, g, m, v, classes), bounds = fx.finite_case(L.P, 3, every)
        for which_bound, b in bounds.items():
            if which_bound == "inf":       # (a factor of 1 either way: the division is all that is left, and it is the same one)
                continue
            kw.update(world=3, max_norm=b)
            assert differs(mut.step(p, g, m, v, **kw), plain.step(p, g, m, v, **kw), classes == "ordinary")
