"""The population entry points' C ABI without a GPU: the four symbols are exported beside an unchanged ABI version, the per-member
workspace stride is what the header promises, and every refusal the learner calls make before they look up the device (and the
rollout call's null handle) returns its code with the function's name in tb_last_error()."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS, NET_DEFAULT, NET_MLP64, NET_TUNED  # noqa: E402

PAIRS = [(ENV_SWING, NET_DEFAULT), (ENV_SWING, NET_MLP64), (ENV_TENNIS, NET_DEFAULT), (ENV_TENNIS, NET_TUNED)]
INVAL, PARAMS = -1, -3


@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return load_library()


def test_symbols_are_exported_and_the_abi_version_did_not_move(lib):
    for name in ("tb_policy_rollout_members", "tb_ppo_members_workspace_stride_bytes", "tb_ppo_grad_members", "tb_ppo_apply_members"):
        assert hasattr(lib, name), name
    assert lib.tb_abi_version() == 4


@pytest.mark.parametrize("kind,net", PAIRS)
@pytest.mark.parametrize("batch", [2, 256, 257, 1100])
def test_workspace_stride_is_a_multiple_of_8_and_holds_one_learners_workspace(lib, kind, net, batch):
    stride, one = lib.tb_ppo_members_workspace_stride_bytes(kind, net, batch), lib.tb_ppo_workspace_bytes_net(kind, net, batch)
    assert one > 0 and stride >= one and stride % 8 == 0 and stride - one < 8


def test_workspace_stride_refusals(lib):
    assert lib.tb_ppo_members_workspace_stride_bytes(ENV_SWING, NET_DEFAULT, 1) == INVAL
    assert lib.tb_ppo_members_workspace_stride_bytes(ENV_SWING, NET_TUNED, 256) == PARAMS
    assert lib.tb_ppo_members_workspace_stride_bytes(ENV_TENNIS, NET_MLP64, 256) == PARAMS


def test_rollout_members_refuses_a_null_handle_by_name(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tb_policy_rollout_members(None, 0, 4, p, 1, 16, 16, p, p, p, p, p, p, p, p, None, 1, 0, None) == INVAL
    assert b"tb_policy_rollout_members" in lib.tb_last_error()


class Call:
    """valid arguments of the two learner calls (host memory stands in: every refusal below comes before the device is looked up)"""

    def __init__(self, lib, kind=ENV_SWING, net=NET_DEFAULT, batch=64, M=3):
        self.lib, self.kind, self.net, self.batch, self.M = lib, kind, net, batch, M
        self.P = lib.tb_ppo_param_floats_net(kind, net)
        self.stride = lib.tb_ppo_members_workspace_stride_bytes(kind, net, batch)
        self.buf = (ctypes.c_double * 64)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p).value
        assert self.p % 8 == 0

    def grad(self, **kw):
        a = dict(kind=self.kind, net=self.net, obs=self.p, act=self.p, old_logp=self.p, adv=self.p, ret=self.p, n_rows=1000, idx=self.p, idx_stride=self.batch,
                 batch=self.batch, M=self.M, params=self.p, param_stride=self.P, P=self.P, hp=self.p, ws=self.p, ws_bytes=self.M * self.stride)
        a.update(kw)
        return self.lib.tb_ppo_grad_members(a["kind"], a["net"], 0, None, a["obs"], a["act"], a["old_logp"], a["adv"], a["ret"], a["n_rows"], a["idx"], a["idx_stride"],
                                            a["batch"], a["M"], a["params"], a["param_stride"], a["P"], a["hp"], a["ws"], a["ws_bytes"])

    def apply(self, **kw):
        a = dict(kind=self.kind, net=self.net, ws=self.p, ws_bytes=self.M * self.stride, batch=self.batch, M=self.M, params=self.p, grad=self.p, m=self.p, v=self.p,
                 param_stride=self.P, P=self.P, stats=self.p, hp=self.p, step=2)
        a.update(kw)
        return self.lib.tb_ppo_apply_members(a["kind"], a["net"], 0, None, a["ws"], a["ws_bytes"], a["batch"], a["M"], a["params"], a["grad"], a["m"], a["v"],
                                             a["param_stride"], a["P"], a["stats"], a["hp"], 0.5, 0.9, 0.999, 1e-5, a["step"])


GRAD_REFUSALS = [
    (dict(M=0), INVAL), (dict(M=65536, ws_bytes=1 << 40), INVAL), (dict(batch=1), INVAL),
    (dict(obs=None), INVAL), (dict(act=None), INVAL), (dict(old_logp=None), INVAL), (dict(adv=None), INVAL), (dict(ret=None), INVAL), (dict(idx=None), INVAL),
    (dict(params=None), INVAL), (dict(hp=None), INVAL), (dict(ws=None), INVAL),
    (dict(obs=2), INVAL), (dict(params=6), INVAL),              # floats: 4-byte alignment
    (dict(idx=4), INVAL), (dict(ws=12), INVAL), (dict(hp=20), INVAL),   # idx, workspace, hp: 8-byte alignment
    (dict(idx_stride=63), INVAL), (dict(param_stride=10), INVAL),
    (dict(ws_bytes=0), INVAL), (dict(P=7), INVAL), (dict(n_rows=0), INVAL),
    (dict(net=NET_TUNED), PARAMS), (dict(kind=ENV_TENNIS, net=NET_MLP64), PARAMS),
]
APPLY_REFUSALS = [
    (dict(M=0), INVAL), (dict(M=65536, ws_bytes=1 << 40), INVAL), (dict(batch=1), INVAL),
    (dict(params=None), INVAL), (dict(grad=None), INVAL), (dict(m=None), INVAL), (dict(v=None), INVAL), (dict(stats=None), INVAL), (dict(hp=None), INVAL),
    (dict(ws=None), INVAL),
    (dict(grad=2), INVAL), (dict(stats=6), INVAL), (dict(ws=12), INVAL), (dict(hp=20), INVAL),
    (dict(param_stride=10), INVAL), (dict(ws_bytes=0), INVAL), (dict(P=7), INVAL), (dict(step=0), INVAL),
    (dict(net=NET_TUNED), PARAMS), (dict(kind=ENV_TENNIS, net=NET_MLP64), PARAMS),
]


def _absolute(call, kw):
    """small integers stand for misaligned addresses: base + that many bytes"""
    return {k: (call.p + v if k in ("obs", "act", "old_logp", "adv", "ret", "idx", "params", "hp", "ws", "grad", "m", "v", "stats") and isinstance(v, int) else v)
            for k, v in kw.items()}


@pytest.mark.parametrize("kw,code", GRAD_REFUSALS)
def test_grad_members_refusals_come_by_name_before_the_device(lib, kw, code):
    call = Call(lib)
    kw = _absolute(call, kw)
    if "ws_bytes" in kw and kw["ws_bytes"] == 0:
        kw["ws_bytes"] = call.M * call.stride - 1       # one byte short of n_members * stride
    assert call.grad(**kw) == code, kw
    assert b"tb_ppo_grad_members" in lib.tb_last_error()


@pytest.mark.parametrize("kw,code", APPLY_REFUSALS)
def test_apply_members_refusals_come_by_name_before_the_device(lib, kw, code):
    call = Call(lib)
    kw = _absolute(call, kw)
    if "ws_bytes" in kw and kw["ws_bytes"] == 0:
        kw["ws_bytes"] = call.M * call.stride - 1
    assert call.apply(**kw) == code, kw
    assert b"tb_ppo_apply_members" in lib.tb_last_error()


def test_the_python_side_granule_is_the_librarys(lib):
    from tennisbot_rl_amd import population
    assert population.MEMBER_GRANULE == lib.tb_policy_member_granule()
    assert ctypes.sizeof(ctypes.c_float) * len(population.HP_COLUMNS) == 16   # TbPpoMemberHp
