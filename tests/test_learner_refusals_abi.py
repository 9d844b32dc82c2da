"""The single learners' refusals without a GPU: tb_ppo_grad_net, tb_ppo_apply_net, tb_trpo_fvp_net, tb_trpo_search_net, tb_ppo_gae and
tb_trpo_returns, and the null handle of the three whole-episode population calls. Host memory stands in for device memory: every case
has ONE fault, is refused before the device is looked up, and returns its code with tb_last_error() beginning with the entry point's
name -- the single forms' is the un-netted one (tb_ppo_grad, not tb_ppo_grad_net). No case here is a valid call: nothing is launched."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED  # noqa: E402

PAIRS = [(ENV_SWING, NET_DEFAULT), (ENV_SWING, NET_MLP64), (ENV_TENNIS, NET_DEFAULT), (ENV_TENNIS, NET_TUNED)]
TRPO_PAIRS = [p for p in PAIRS if p[1] != NET_TUNED]
UNBUILT = [(ENV_SWING, NET_TUNED), (ENV_TENNIS, NET_MLP64), (ENV_SWING, 9), (ENV_TENNIS, -1)]
INVAL, PARAMS, UNSUPPORTED = -1, -3, -4
REDUCE, STEP, VALUE_ONLY = 1, 2, 4
BATCH, N_IDX, N_CAND, T, N = 300, 300, 8, 5, 100


@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return load_library()


_BUF = (ctypes.c_double * 128)()
P0 = ctypes.cast(_BUF, ctypes.c_void_p).value  # an 8-byte aligned address; P0 + 512 is a second one
assert P0 % 8 == 0


class Call:
    """one entry point, the names of its arguments in order, and a valid value for each"""

    def __init__(self, lib, name, says, order, **valid):
        self.fn, self.says, self.order, self.valid, self.lib = getattr(lib, name), says.encode() + b":", order.split(), valid, lib
        assert set(self.order) == set(valid), set(self.order) ^ set(valid)

    def refused(self, code, **fault):
        """pointers are given as a byte offset from their valid value (None: null), everything else as the value itself"""
        a = dict(self.valid)
        for k, v in fault.items():
            assert k in a, k
            a[k] = v if v is None or not k.startswith("p_") else a[k] + v
        assert self.fn(*[a[k] for k in self.order]) == code, fault
        err = self.lib.tb_last_error()
        assert err.startswith(self.says), (fault, err)


def grad_call(lib, kind, net):
    P = lib.tb_ppo_param_floats_net(kind, net) if (kind, net) in PAIRS else 7
    wb = lib.tb_ppo_workspace_bytes_net(kind, net, BATCH) if (kind, net) in PAIRS else 1 << 30
    return Call(lib, "tb_ppo_grad_net", "tb_ppo_grad", "kind net device stream p_obs p_act p_old_logp p_adv p_ret n_rows p_idx batch p_params P clip vf p_ws ws_bytes",
                kind=kind, net=net, device=0, stream=None, p_obs=P0, p_act=P0, p_old_logp=P0, p_adv=P0, p_ret=P0, n_rows=1000, p_idx=P0, batch=BATCH, p_params=P0, P=P,
                clip=0.2, vf=0.5, p_ws=P0, ws_bytes=wb)


def apply_call(lib, kind, net, phases=REDUCE | STEP):
    P = lib.tb_ppo_param_floats_net(kind, net) if (kind, net) in PAIRS else 7
    wb = lib.tb_ppo_workspace_bytes_net(kind, net, BATCH) if (kind, net) in PAIRS else 1 << 30
    return Call(lib, "tb_ppo_apply_net", "tb_ppo_apply", "kind net device stream phases p_ws ws_bytes batch p_params p_grad p_m p_v P p_stats ent max_norm world lr b1 b2 eps step",
                kind=kind, net=net, device=0, stream=None, phases=phases, p_ws=P0, ws_bytes=wb, batch=BATCH, p_params=P0, p_grad=P0, p_m=P0, p_v=P0, P=P, p_stats=P0,
                ent=0.0, max_norm=0.5, world=1, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5, step=1)


def fvp_call(lib, kind, net):
    ok = (kind, net) in TRPO_PAIRS
    P = lib.tb_ppo_param_floats_net(kind, net) if ok else 7
    wb = lib.tb_trpo_fvp_workspace_bytes_net(kind, net, N_IDX) if ok else 1 << 30
    return Call(lib, "tb_trpo_fvp_net", "tb_trpo_fvp", "kind net device stream p_obs n_rows p_idx n_idx p_params p_vec P damping p_out p_ws ws_bytes",
                kind=kind, net=net, device=0, stream=None, p_obs=P0, n_rows=1000, p_idx=P0, n_idx=N_IDX, p_params=P0, p_vec=P0, P=P, damping=0.1, p_out=P0 + 512, p_ws=P0,
                ws_bytes=wb)


def search_call(lib, kind, net):
    ok = (kind, net) in TRPO_PAIRS
    P = lib.tb_ppo_param_floats_net(kind, net) if ok else 7
    wb = lib.tb_trpo_search_workspace_bytes_net(kind, net, BATCH, N_CAND) if ok else 1 << 30
    return Call(lib, "tb_trpo_search_net", "tb_trpo_search",
                "kind net device stream p_obs p_act p_old_logp p_adv n_rows p_idx batch p_params p_dir P p_steps n_cand p_out p_ws ws_bytes",
                kind=kind, net=net, device=0, stream=None, p_obs=P0, p_act=P0, p_old_logp=P0, p_adv=P0, n_rows=1000, p_idx=P0, batch=BATCH, p_params=P0, p_dir=P0, P=P,
                p_steps=P0, n_cand=N_CAND, p_out=P0, p_ws=P0, ws_bytes=wb)


def gae_call(lib):
    return Call(lib, "tb_ppo_gae", "tb_ppo_gae", "kind device stream T n p_rew rs p_done ds p_val p_last gamma lam p_adv p_ret",
                kind=ENV_SWING, device=0, stream=None, T=T, n=N, p_rew=P0, rs=0, p_done=P0, ds=0, p_val=P0, p_last=P0, gamma=0.99, lam=0.95, p_adv=P0, p_ret=P0)


def returns_call(lib):
    return Call(lib, "tb_trpo_returns", "tb_trpo_returns", "kind device stream T n p_rew rs p_done ds discount p_ret p_idx p_count p_ws ws_bytes",
                kind=ENV_SWING, device=0, stream=None, T=T, n=N, p_rew=P0, rs=0, p_done=P0, ds=0, discount=0.98, p_ret=P0, p_idx=P0, p_count=P0, p_ws=P0,
                ws_bytes=lib.tb_trpo_returns_workspace_bytes(T, N))


def _ids(faults):
    return ["-".join("%s=%s" % kv for kv in f.items()) for f in faults]


GRAD_FAULTS = [dict(p_obs=None), dict(p_act=None), dict(p_old_logp=None), dict(p_adv=None), dict(p_ret=None), dict(p_idx=None), dict(p_params=None), dict(p_ws=None),
               dict(P=-1), dict(n_rows=0), dict(batch=1),
               dict(p_obs=2), dict(p_act=2), dict(p_old_logp=2), dict(p_adv=2), dict(p_ret=2), dict(p_params=2),  # floats: 4-byte alignment
               dict(p_idx=4), dict(p_ws=4),                                                                      # idx, workspace: 8-byte alignment
               dict(ws_bytes=-1)]


@pytest.mark.parametrize("kind,net", PAIRS)
@pytest.mark.parametrize("fault", GRAD_FAULTS, ids=_ids(GRAD_FAULTS))
def test_ppo_grad_refusals(lib, kind, net, fault):
    call = grad_call(lib, kind, net)
    fault = {k: call.valid[k] + v if k in ("P", "ws_bytes") else v for k, v in fault.items()}  # (one off the valid value)
    call.refused(INVAL, **fault)


@pytest.mark.parametrize("make", [grad_call, apply_call, fvp_call, search_call], ids=["grad", "apply", "fvp", "search"])
def test_an_unknown_kind_and_an_unbuilt_pair(lib, make):
    make(lib, 7, NET_DEFAULT).refused(INVAL)
    for kind, net in UNBUILT:
        make(lib, kind, net).refused(PARAMS)


APPLY_FAULTS = [dict(phases=0), dict(phases=8), dict(phases=REDUCE | 8), dict(phases=REDUCE | STEP | 16),
                dict(p_params=None), dict(p_grad=None), dict(P=-1),
                dict(p_params=2), dict(p_grad=2), dict(p_m=2), dict(p_v=2), dict(p_stats=2),
                dict(p_ws=None), dict(p_stats=None), dict(batch=1), dict(p_ws=4), dict(ws_bytes=-1),  # TB_PPO_REDUCE's
                dict(p_m=None), dict(p_v=None), dict(world=0), dict(step=0)]                         # TB_PPO_STEP's


@pytest.mark.parametrize("kind,net", PAIRS)
@pytest.mark.parametrize("fault", APPLY_FAULTS, ids=_ids(APPLY_FAULTS))
def test_ppo_apply_refusals(lib, kind, net, fault):
    call = apply_call(lib, kind, net)
    fault = {k: call.valid[k] + v if k in ("P", "ws_bytes") else v for k, v in fault.items()}
    call.refused(INVAL, **fault)


@pytest.mark.parametrize("kind,net", PAIRS)
def test_ppo_apply_refuses_each_phase_alone_for_what_it_needs(lib, kind, net):
    reduce_only, step_only = apply_call(lib, kind, net, REDUCE), apply_call(lib, kind, net, STEP)
    for fault in (dict(p_ws=None), dict(p_stats=None), dict(batch=1), dict(p_ws=4), dict(ws_bytes=reduce_only.valid["ws_bytes"] - 1)):
        reduce_only.refused(INVAL, **fault)
    for fault in (dict(p_m=None), dict(p_v=None), dict(world=0), dict(step=0)):
        step_only.refused(INVAL, **fault)


@pytest.mark.parametrize("kind,net", [p for p in PAIRS if p[1] != NET_TUNED])
def test_ppo_apply_refuses_value_only_without_a_phase(lib, kind, net):
    apply_call(lib, kind, net, VALUE_ONLY).refused(INVAL)


@pytest.mark.parametrize("phases", [REDUCE | VALUE_ONLY, STEP | VALUE_ONLY, REDUCE | STEP | VALUE_ONLY])
def test_ppo_apply_has_no_value_only_on_the_tuned_net(lib, phases):
    apply_call(lib, ENV_TENNIS, NET_TUNED, phases).refused(UNSUPPORTED)


FVP_FAULTS = [dict(p_obs=None), dict(p_idx=None), dict(p_params=None), dict(p_vec=None), dict(p_out=None), dict(p_ws=None),
              dict(P=-1), dict(n_rows=0), dict(n_idx=0),
              dict(p_obs=2), dict(p_params=2), dict(p_vec=2), dict(p_out=2), dict(p_idx=4), dict(p_ws=4),
              dict(p_out=-512),   # out_dev == vec_dev
              dict(ws_bytes=-1)]


@pytest.mark.parametrize("kind,net", TRPO_PAIRS)
@pytest.mark.parametrize("fault", FVP_FAULTS, ids=_ids(FVP_FAULTS))
def test_trpo_fvp_refusals(lib, kind, net, fault):
    call = fvp_call(lib, kind, net)
    fault = {k: call.valid[k] + v if k in ("P", "ws_bytes") else v for k, v in fault.items()}
    call.refused(INVAL, **fault)


SEARCH_FAULTS = [dict(p_obs=None), dict(p_act=None), dict(p_old_logp=None), dict(p_adv=None), dict(p_idx=None), dict(p_params=None), dict(p_dir=None), dict(p_steps=None),
                 dict(p_out=None), dict(p_ws=None),
                 dict(P=-1), dict(n_rows=0), dict(batch=1), dict(n_cand=0), dict(n_cand=65),
                 dict(p_obs=2), dict(p_act=2), dict(p_old_logp=2), dict(p_adv=2), dict(p_params=2), dict(p_dir=2), dict(p_steps=2),
                 dict(p_idx=4), dict(p_ws=4), dict(p_out=4),
                 dict(ws_bytes=-1)]


@pytest.mark.parametrize("kind,net", TRPO_PAIRS)
@pytest.mark.parametrize("fault", SEARCH_FAULTS, ids=_ids(SEARCH_FAULTS))
def test_trpo_search_refusals(lib, kind, net, fault):
    call = search_call(lib, kind, net)
    fault = {k: call.valid[k] + v if k in ("P", "ws_bytes") else v for k, v in fault.items()}
    call.refused(INVAL, **fault)


def test_the_trpo_calls_refuse_the_tuned_net_by_their_own_name(lib):
    for make in (fvp_call, search_call):
        call = make(lib, ENV_TENNIS, NET_TUNED)
        call.refused(PARAMS)
        assert b"TB_NET_TUNED is not built for the TRPO kernels" in lib.tb_last_error()


GAE_FAULTS = [dict(kind=7), dict(p_rew=None), dict(p_done=None), dict(p_val=None), dict(p_last=None), dict(p_adv=None), dict(p_ret=None),
              dict(T=0), dict(n=0),
              dict(p_rew=2), dict(p_val=2), dict(p_last=2), dict(p_adv=2), dict(p_ret=2),
              dict(rs=4 * N + 2),     # not a multiple of 4 bytes
              dict(rs=4 * (N - 1)),   # shorter than n_envs floats
              dict(ds=N - 1)]         # shorter than n_envs bytes


@pytest.mark.parametrize("fault", GAE_FAULTS, ids=_ids(GAE_FAULTS))
def test_ppo_gae_refusals(lib, fault):
    gae_call(lib).refused(INVAL, **fault)


RETURNS_FAULTS = [dict(kind=7), dict(p_rew=None), dict(p_done=None), dict(p_ret=None), dict(p_idx=None), dict(p_count=None), dict(p_ws=None),
                  dict(T=0), dict(n=0),
                  dict(p_rew=2), dict(p_ret=2), dict(p_idx=4), dict(p_count=4), dict(p_ws=4),
                  dict(rs=4 * N + 2), dict(rs=4 * (N - 1)), dict(ds=N - 1),
                  dict(T=1 << 20, n=64 * 2048, ws_bytes=1 << 62),        # n_steps * ceil(n_envs / 64) = 2^31
                  dict(T=1 << 20, n=64 * 2047 + 1, ws_bytes=1 << 62),    # ... the same with a ragged last chunk
                  dict(ws_bytes=0)]


@pytest.mark.parametrize("fault", RETURNS_FAULTS, ids=_ids(RETURNS_FAULTS))
def test_trpo_returns_refusals(lib, fault):
    call = returns_call(lib)
    if fault.get("ws_bytes") == 0:
        fault = dict(ws_bytes=call.valid["ws_bytes"] - 1)
    call.refused(INVAL, **fault)


def test_the_whole_episode_population_calls_refuse_a_null_handle_by_name(lib):
    assert lib.tb_policy_evaluate_members(None, NET_DEFAULT, P0, 1, 16, 16, P0, P0, 1, 0, None) == INVAL
    assert lib.tb_last_error().startswith(b"tb_policy_evaluate_members:")
    assert lib.tb_sac_evaluate_members(None, P0, 1, 16, 16, P0, P0, 1, 0, None, None) == INVAL
    assert lib.tb_last_error().startswith(b"tb_sac_evaluate_members:")
    assert lib.tb_es_evaluate(None, P0, 1, 4, 1, P0, P0, None, None) == INVAL
    assert lib.tb_last_error().startswith(b"tb_es_evaluate:")
