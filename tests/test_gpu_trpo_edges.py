"""tb_trpo_fvp and tb_trpo_search on the weight regimes of tests/learner_edge_fixtures.py (tanh saturated, tanh overflowing,
log_std at -5 / +2), both env kinds, m = 17, 129 and 257 rows through an index vector with a repeat and two out-of-range entries,
against tests/trpo_reference.py within ppo_reference.MULTIPLE float32-twin errors per tensor; and the line search where candidates
are not finite: two giant first steps (the later candidates must be untouched and the accepted one the reference's), every step
giant (nothing accepted), and a whole FusedTRPO.policy_step whose kl_delta makes every step infinite: theta keeps its bits.
The largest ratios are printed at the end of the module and quoted in DESIGN.md."""
import numpy as np
import pytest

import learner_edge_fixtures as lf
import trpo_reference as tr
from test_ppo_reference import make_policy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("trpo edges (gpu): largest %s = %.3g" % (k, RATIOS[k]))


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def h(x):
    return x.detach().cpu().numpy().copy()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def make_trpo(torch, f, **hp):
    from tennisbot_rl_amd.trpo import FusedTRPO
    policy = make_policy(f.arch, f.kind)
    policy.load_state_dict({k: torch.from_numpy(v.astype(np.float32)) for k, v in f.P.items()})
    policy = policy.to(DEV)
    opt = torch.optim.Adam(policy.parameters(), lr=f.hp["learning_rate"], eps=1e-5)
    return FusedTRPO(f.kind, policy, opt, dict(f.hp, **hp), torch.device(DEV))


@pytest.mark.parametrize("which", lf.WEIGHT_REGIMES)
@pytest.mark.parametrize("kname", list(lf.CASE))
def test_fvp_on_the_edge_fixture(torch, kname, which):
    f = lf.build(kname, which)
    L = make_trpo(torch, f)
    obs = f.data[0][:lf.N_ROWS]
    obs_d = dev(torch, obs)
    vec, v = lf.fvp_vector(f.P)
    assert len(vec) == L.n_params and np.all(vec != 0.0)
    vec_d = dev(torch, vec)
    d32 = np.float32(tr.CG_DAMPING)
    mask = h(L.mask) != 0
    for m in lf.SIZES:
        tag = "%s %s fvp m = %d" % (kname, which, m)
        idx, rows = lf.gpu_rows(f, "fvp", m)
        idx_d = dev(torch, idx)
        out = [torch.full((L.n_params,), 7.0, device=DEV) for _ in range(2)]
        L.fvp(obs_d, idx_d.data_ptr(), m, vec_d, out[0])
        L.fvp(obs_d, idx_d.data_ptr(), m, vec_d, out[1])
        assert torch.equal(out[0], out[1]), "%s: a second run gave other bits" % tag
        got = h(out[0])
        assert np.isfinite(got).all() and not got[~mask].any()
        want, twin = tr.fvp(f.P, obs[rows], v, float(d32)), tr.fvp(f.P, obs[rows], v, float(d32), np.float32)
        gd, vd = tr.theta_of(tr.split_flat(got, f.P)), tr.split_flat(vec, f.P)
        r = lf.ratios(gd, want, twin)
        worst = max(r, key=r.get)
        print("%s: %.3g twin errors (%s)" % (tag, r[worst], worst))
        if which == "overflow":       # h = +-1 exactly: nothing flows through units 0 and 1 of the first layer, F v's slots are 0
            for k in ("policy_net.0.weight", "policy_net.0.bias"):
                assert np.array_equal(bits(gd[k][:2]), bits(d32 * vd[k][:2])), "%s: %s units 0 / 1 are not fl(damping v)" % (tag, k)
        note("FVP error / twin error, %s" % which, lf.check(tag, gd, want, twin))


def run_search(torch, L, f, rows, idx, case):
    data, x, steps = lf.search_case(f, rows, case)
    host = [a[:lf.N_ROWS].copy() for a in f.data[:4]]
    if case == "inf_ratio":
        host[2][lf.inf_ratio_row(f, rows)] = lf.INF_OLD_LOGP
    arrays = tuple(dev(torch, a) for a in host)
    idx_d, x_d, steps_d = dev(torch, idx), dev(torch, tr.join_flat(x, f.P, np.float32)), dev(torch, steps)
    got_t = L.search(arrays, lf.N_ROWS, idx_d.data_ptr(), len(idx), x_d, steps_d)
    torch.cuda.synchronize()
    s64 = steps.astype(np.float64)
    with np.errstate(all="ignore"):
        want, twin = tr.search_table(f.P, x, s64, *data), tr.search_table(f.P, x, s64, *data, np.float32)
    return got_t, want, twin


@pytest.mark.parametrize("which", lf.WEIGHT_REGIMES)
@pytest.mark.parametrize("kname", list(lf.CASE))
def test_search_on_the_edge_fixture(torch, kname, which):
    from tennisbot_rl_amd.trpo import select_candidate
    f = lf.build(kname, which)
    L = make_trpo(torch, f)
    for m in lf.SIZES:
        idx, rows = lf.gpu_rows(f, "search", m)
        # a ratio that overflows: L_k = +inf beside an acceptable KL_k. Only select_candidate's finiteness test rejects it
        got_t, want, twin = run_search(torch, L, f, rows, idx, "inf_ratio")
        got = h(got_t)
        assert (got[:, 0] == np.inf).all() and (twin[:, 0] == np.inf).all() and np.isfinite(got[:, 1]).all() and (got[:, 1] <= tr.KL_DELTA).any(), got
        note("search error / twin error, %s" % which, lf.check("%s %s search m = %d inf_ratio KL" % (kname, which, m), {"KL": got[:, 1]}, {"KL": want[:, 1]}, {"KL": twin[:, 1]}))
        assert int(select_candidate(torch, got_t, tr.KL_DELTA)) == -1 == tr.select(got) == tr.select(want)
        for case in ("kl", "overflow_head", "all_nonfinite"):
            tag = "%s %s search m = %d %s" % (kname, which, m, case)
            got_t, want, twin = run_search(torch, L, f, rows, idx, case)
            got = h(got_t)
            fin = lf.finite_rows(twin)
            head = {"kl": 0, "overflow_head": 2, "all_nonfinite": tr.CANDIDATES}[case]
            assert not fin[:head].any() and fin[head:].all(), (tag, twin)
            k_dev = int(select_candidate(torch, got_t, tr.KL_DELTA))
            if fin.any():
                assert tr.threshold_margins(want[fin], twin[fin]).min() > lf.MARGIN, tag
                r = lf.ratios(lf.columns(got[fin]), lf.columns(want[fin]), lf.columns(twin[fin]))
                worst = max(r, key=r.get)
                print("%s: %.3g twin errors (%s); accepted %d" % (tag, r[worst], worst, k_dev))
            # a candidate that is not finite in the twin is rejected on the device too: as non-finite, or by its KL
            for k in np.nonzero(~fin)[0]:
                assert not (np.isfinite(got[k]).all() and got[k, 1] <= tr.KL_DELTA and got[k, 0] >= 0.0), "%s: candidate %d would be accepted: %s" % (tag, k, got[k])
            assert k_dev == tr.select(want) == tr.select(got), (tag, got, want)
            if case == "all_nonfinite":
                assert k_dev == -1
            if fin.any():
                note("search error / twin error, %s" % which, lf.check(tag, lf.columns(got[fin]), lf.columns(want[fin]), lf.columns(twin[fin])))


@pytest.mark.parametrize("kname", list(lf.CASE))
def test_policy_step_with_every_candidate_infinite_keeps_theta(torch, kname):
    """kl_delta = 1e90: beta = sqrt(2 delta / x^T F x) exceeds float32 for every candidate, theta + inf x is not finite, every row
    of the table is rejected and theta keeps its bits"""
    f = lf.build(kname, "log_std")
    L = make_trpo(torch, f, kl_delta=1e90)
    arrays = tuple(dev(torch, x[:lf.N_ROWS]) for x in f.data)
    rows_d = torch.arange(lf.N_ROWS, device=DEV)
    before = h(L.flat)
    k, Lk, KLk = L.policy_step(arrays, lf.N_ROWS, rows_d.data_ptr(), rows_d.data_ptr(), lf.N_ROWS)
    torch.cuda.synchronize()
    table = h(L.table)
    assert int(k) == -1 and not np.isfinite(table).all(1).any(), table
    after = h(L.flat)
    assert np.isfinite(after).all() and np.array_equal(bits(after), bits(before)), "a rejected step moved theta"
