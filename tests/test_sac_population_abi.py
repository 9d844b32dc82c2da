"""The SAC / TQC population entry points' C ABI without a GPU: the eleven symbols are exported beside an unchanged ABI version, the
per-member workspace stride is what the header promises, and every refusal the calls make before they look up the device returns its
code with the entry point's name in tb_last_error(). Host addresses stand in for device memory: every call below is refused, so
none is ever dereferenced."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tennisbot_rl_amd.params import ENV_SWING, ENV_TENNIS  # noqa: E402

INVAL, PARAMS = -1, -3
ALGOS = ("tb_sac_", "tb_tqc_")
STAGES = ("actor_forward_members", "targets_members", "critic_grad_members", "actor_grad_members")
FAR = 1 << 26   # bytes between the stand-in addresses of two arrays: more than any population below spans


@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return load_library()


def test_symbols_are_exported_and_the_abi_version_did_not_move(lib):
    for prefix in ALGOS:
        for name in STAGES + ("members_workspace_stride_bytes",):
            assert hasattr(lib, prefix + name), prefix + name
    assert hasattr(lib, "tb_sac_adam_members")
    assert lib.tb_abi_version() == 4


def test_declared_signatures(lib):
    """the argument lists of include/tb_stepper.h, as stepper.load_library declares them: the two algorithms' twins agree, and each
    members stage is its single-member stage plus the member count and one stride per per-member array"""
    sz, vp, i32, i64 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    extra = {"actor_forward_members": 6, "targets_members": 6, "critic_grad_members": 4, "actor_grad_members": 4}   # n_members + strides (+ hp in the targets, - gamma)
    for stage in STAGES:
        sac, tqc = getattr(lib, "tb_sac_" + stage), getattr(lib, "tb_tqc_" + stage)
        assert sac.argtypes == tqc.argtypes and sac.restype == tqc.restype == i32
        single = getattr(lib, "tb_sac_" + stage[:-len("_members")])
        assert len(sac.argtypes) == len(single.argtypes) + extra[stage], stage
        assert sac.argtypes[:3] == [i32, i32, vp] and sac.argtypes[-2:] == [vp, sz]
    assert lib.tb_sac_targets_members.argtypes.count(ctypes.c_float) == 0   # gamma comes from the hp row
    assert lib.tb_sac_members_workspace_stride_bytes.argtypes == [i32, i32] and lib.tb_sac_members_workspace_stride_bytes.restype == i64
    assert lib.tb_tqc_members_workspace_stride_bytes.argtypes == [i32, i32] and lib.tb_tqc_members_workspace_stride_bytes.restype == i64
    assert len(lib.tb_sac_adam_members.argtypes) == 16 and lib.tb_sac_adam_members.argtypes.count(ctypes.c_float) == 3   # betas and eps: lr and tau are per member


def header_prototypes():
    """name -> (restype, [argtypes]) of every tb_sac_ / tb_tqc_ prototype of include/tb_stepper.h whose name holds `members`, its C
    types read as ctypes: any pointer is a void pointer, the rest by name"""
    import re
    text = open(os.path.join(ROOT, "include", "tb_stepper.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    scalars = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
               "double": ctypes.c_double, "uint64_t": ctypes.c_uint64}
    out = {}
    for ret, name, args in re.findall(r"^(int|long long)\s+(tb_(?:sac|tqc)_\w*members\w*)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S):
        types = []
        for arg in args.split(","):
            arg = " ".join(arg.split())
            if "*" in arg:
                types.append(ctypes.c_void_p)
            else:
                types.append(scalars[arg.replace("const ", "").rsplit(" ", 1)[0]])   # the type is everything before the parameter's name
        out[name] = (scalars[ret], types)
    return out


def test_declared_signatures_are_the_headers(lib):
    """what stepper.load_library declares for each members entry is include/tb_stepper.h's prototype, argument by argument: a wrong
    declaration shared by both algorithms' twins would not pass"""
    protos = header_prototypes()
    names = [p + s for p in ALGOS for s in STAGES + ("members_workspace_stride_bytes",)] + ["tb_sac_adam_members"]
    assert sorted(n for n in protos if n != "tb_sac_evaluate_members") == sorted(names)   # (tb_sac_evaluate_members: an earlier entry, declared with a handle)
    for name in names:
        f, (restype, argtypes) = getattr(lib, name), protos[name]
        assert f.restype == restype, name
        assert list(f.argtypes) == argtypes, name


@pytest.mark.parametrize("prefix", ALGOS)
@pytest.mark.parametrize("kind", [ENV_SWING, ENV_TENNIS])
@pytest.mark.parametrize("batch", [1, 2, 17, 256, 257, 1100])
def test_workspace_stride_is_a_multiple_of_8_and_holds_one_learners_workspace(lib, prefix, kind, batch):
    stride, one = getattr(lib, prefix + "members_workspace_stride_bytes")(kind, batch), getattr(lib, prefix + "workspace_bytes")(kind, batch)
    assert one > 0 and stride >= one and stride % 8 == 0 and stride - one < 8


@pytest.mark.parametrize("prefix", ALGOS)
def test_workspace_stride_refusals(lib, prefix):
    f = getattr(lib, prefix + "members_workspace_stride_bytes")
    for kind, batch in ((2, 16), (-1, 16), (ENV_SWING, 0)):
        assert f(kind, batch) == INVAL
        assert (prefix + "members_workspace_stride_bytes").encode() in lib.tb_last_error()


def test_the_python_sides_hp_row_is_the_headers(lib):
    from tennisbot_rl_amd import sac_population as sp
    assert ctypes.sizeof(ctypes.c_float) * sp.HP_WIDTH == 32 and sp.HP_WIDTH & (sp.HP_WIDTH - 1) == 0   # TbSacMemberHp: a power of two
    assert sp.HP_COLUMNS == ("lr_actor", "lr_critic", "lr_ent", "gamma", "tau") and (sp.LR_ACTOR, sp.LR_CRITIC, sp.LR_ENT) == (0, 1, 2)
    assert sp.MAX_MEMBERS == 32767 and 2 * sp.MAX_MEMBERS <= 65535   # (member, net) on the grid's z axis


class Call:
    """valid arguments of the members calls, by name; ORDER lists each entry point's argument names in the header's order"""

    ORDER = {
        "actor_forward_members": "kind device stream obs n_rows idx idx_stride batch M actor actor_stride eps eps_stride act act_stride logp logp_stride ws ws_bytes",
        "targets_members": "kind device stream next_obs reward done n_rows idx idx_stride batch M actor actor_stride target critic_stride lec eps eps_stride hp y y_stride ws ws_bytes",
        "critic_grad_members": "kind device stream obs action n_rows idx idx_stride batch M critic critic_stride y y_stride grad stats ws ws_bytes",
        "actor_grad_members": "kind device stream batch M actor actor_stride critic critic_stride lec eps eps_stride grad ent_grad stats ws ws_bytes",
    }
    POINTERS = ("obs", "next_obs", "action", "reward", "done", "idx", "actor", "critic", "target", "eps", "act", "logp", "lec", "hp", "y", "grad", "ent_grad", "stats", "ws")

    def __init__(self, lib, prefix, stage, kind=ENV_SWING, batch=17, M=3):
        self.lib, self.prefix, self.stage, self.kind, self.batch, self.M = lib, prefix, stage, kind, batch, M
        self.A = 6 if kind == ENV_SWING else 2
        algo = "tb_sac_" if prefix == "tb_sac_" else "tb_tqc_"
        self.PI, self.Q = getattr(lib, algo + "param_floats")(kind, 0), getattr(lib, algo + "param_floats")(kind, 1)
        self.YW = 1 if prefix == "tb_sac_" else 46
        self.stride = getattr(lib, prefix + "members_workspace_stride_bytes")(kind, batch)
        self.buf = (ctypes.c_double * 8)()
        self.p = ctypes.cast(self.buf, ctypes.c_void_p).value
        assert self.p % 8 == 0

    def defaults(self):
        a = dict(kind=self.kind, device=0, stream=None, n_rows=1000, idx_stride=self.batch, batch=self.batch, M=self.M, actor_stride=self.PI, critic_stride=self.Q,
                 eps_stride=self.batch * self.A, act_stride=self.batch * self.A, logp_stride=self.batch, y_stride=self.batch * self.YW, ws_bytes=self.M * self.stride)
        for k, name in enumerate(self.POINTERS):   # every array at a stand-in address of its own, far from the others
            a[name] = self.p + k * FAR
        return a

    def __call__(self, **kw):
        a = self.defaults()
        a.update(kw)
        return getattr(self.lib, self.prefix + self.stage)(*[a[name] for name in self.ORDER[self.stage].split()])


def _cases(stage):
    """(keywords, code) of every refusal of `stage`; a small integer for a pointer means base + that many bytes (misaligned)"""
    names = Call.ORDER[stage].split()
    out = [(dict(kind=2), INVAL), (dict(kind=-1), INVAL), (dict(M=0), INVAL), (dict(M=32768, ws_bytes=1 << 50), INVAL), (dict(batch=0), INVAL), (dict(batch=-3), INVAL),
           (dict(ws_bytes="short"), PARAMS), (dict(ws_bytes=0), PARAMS)]
    for name in names:
        if name in Call.POINTERS:
            out.append(({name: None}, INVAL))
            if name in ("idx", "stats", "hp", "ws"):
                out.append(({name: 4}, INVAL))    # 8-byte alignment
            else:
                out.append(({name: 2}, INVAL))    # floats: 4-byte alignment
        elif name.endswith("_stride"):
            out.append(({name: "short"}, INVAL))
            out.append(({name: 0}, INVAL))
    if "n_rows" in names:
        out.append((dict(n_rows=0), INVAL))
    if stage == "critic_grad_members":
        out += [(dict(grad="critic"), INVAL), (dict(grad="critic+1row"), INVAL)]
    if stage == "actor_grad_members":
        out += [(dict(grad="actor"), INVAL), (dict(grad="actor+1row"), INVAL)]
    return out


CASES = [(prefix, stage, kw, code) for prefix in ALGOS for stage in STAGES for kw, code in _cases(stage)]


@pytest.mark.parametrize("prefix,stage,kw,code", CASES, ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_stage_refusals_come_by_name_before_the_device(lib, prefix, stage, kw, code):
    call = Call(lib, prefix, stage)
    d, kw = call.defaults(), dict(kw)
    short = dict(idx_stride=call.batch - 1, actor_stride=call.PI - 1, critic_stride=call.Q - 1, eps_stride=call.batch * call.A - 1, act_stride=call.batch * call.A - 1,
                 logp_stride=call.batch - 1, y_stride=call.batch * call.YW - 1, ws_bytes=call.M * call.stride - 1)
    for k, v in list(kw.items()):
        if v == "short":
            kw[k] = short[k]
        elif k in Call.POINTERS and isinstance(v, int):
            kw[k] = d[k] + v
        elif isinstance(v, str):   # a gradient on, or one row into, its parameters
            base = v.split("+")[0]
            kw[k] = d[base] + (4 * (call.PI if base == "actor" else call.Q) if "+" in v else 0)
    assert call(**kw) == code, kw
    assert (prefix + stage).encode() in lib.tb_last_error()


def adam(lib, p, **kw):
    a = dict(params=p, grad=p + FAR, m=p + 2 * FAR, v=p + 3 * FAR, n=1000, stride=1000, M=3, hp=p + 4 * FAR, which=0, step=2, target=p + 5 * FAR)
    a.update(kw)
    return lib.tb_sac_adam_members(0, None, a["params"], a["grad"], a["m"], a["v"], a["n"], a["stride"], a["M"], a["hp"], a["which"], 0.9, 0.999, 1e-8, a["step"], a["target"])


ADAM_REFUSALS = [dict(M=0), dict(M=32768), dict(params=None), dict(grad=None), dict(m=None), dict(v=None), dict(hp=None), dict(n=0), dict(step=0), dict(which=3), dict(which=-1),
                 dict(params=2), dict(grad=2), dict(m=2), dict(v=2), dict(target=2), dict(hp=4), dict(stride=999), dict(stride=0), dict(grad="params"), dict(target="params"),
                 dict(grad="params+1row"), dict(grad=None, m=None, v=None, target=None), dict(grad=None, m=None)]


@pytest.mark.parametrize("kw", ADAM_REFUSALS, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_adam_members_refusals_come_by_name_before_the_device(lib, kw):
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    base = dict(params=p, grad=p + FAR, m=p + 2 * FAR, v=p + 3 * FAR, hp=p + 4 * FAR, target=p + 5 * FAR)
    kw = dict(kw)
    for k, v in list(kw.items()):
        if isinstance(v, str):
            kw[k] = p + (4000 if "+" in v else 0)
        elif k in base and isinstance(v, int):
            kw[k] = base[k] + v
    assert adam(lib, p, **kw) == INVAL, kw
    assert b"tb_sac_adam_members" in lib.tb_last_error()
