"""tb_swing_trace's C ABI, as far as it goes without a GPU: the symbol is exported and declared, its ctypes prototype matches the
declaration, the ABI version is still 4, a null handle is refused with the library's own message before any device is looked for,
and BatchedEnv.trace_step turns a Tennisbot-v0 env away before it calls the library at all."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tb_stepper.h")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return load_library()


def test_the_symbol_is_exported_and_the_abi_version_stays_4(lib):
    assert hasattr(lib, "tb_swing_trace")
    assert ctypes.CDLL(lib._name).tb_swing_trace   # straight from the shared object, not through the prototypes of load_library
    assert lib.tb_abi_version() == 4 and "#define TB_ABI_VERSION 4" in open(HEADER).read()


def test_header_declaration_and_ctypes_prototype_agree(lib):
    text = open(HEADER).read()
    m = re.search(r"int tb_swing_trace\((.*?)\);", text, re.S)
    assert m, "tb_swing_trace is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["h", "words_dev", "done_dev", "n_rows", "actions_dev", "stride", "max_frames", "frames_dev", "n_frames_dev", "reward_dev",
                     "substeps_dev", "done_out_dev", "obs_dev_or_null", "stream"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    want = [i32 if a.split()[0] == "int" and "*" not in a else vp for a in args]
    assert lib.tb_swing_trace.restype is i32 and list(lib.tb_swing_trace.argtypes) == want
    assert "s = 1 .. ns" in text and "1 + (ns - 1) / stride + ((ns - 1) % stride != 0)" in text   # the sampling rule is stated there


def test_a_null_handle_is_refused_with_the_functions_name(lib):
    from tennisbot_rl_amd import stepper
    buf = (ctypes.c_uint32 * 64)()   # host addresses that are never dereferenced: the call is refused before any device is looked for
    p = ctypes.cast(buf, ctypes.c_void_p).value
    rc = lib.tb_swing_trace(None, p, p, 1, p, 8, 2, p, p, p, p, p, p, None)
    assert rc == -1   # TB_E_INVAL
    msg = lib.tb_last_error().decode()
    assert "tb_swing_trace" in msg and "null handle" in msg
    with pytest.raises(stepper.StepperError, match=re.escape(msg)):
        stepper._check(lib, rc, "tb_swing_trace")


def test_trace_step_on_tennisbot_raises_before_any_library_call():
    from tennisbot_rl_amd import stepper
    from tennisbot_rl_amd.params import ENV_TENNIS

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("the library was reached: %s" % name)

    env = object.__new__(stepper.BatchedEnv)   # no GPU here, and none is needed: the refusal touches nothing of the batch
    env.kind, env.L, env._h, env.torch = ENV_TENNIS, NoCalls(), None, NoCalls()
    with pytest.raises(ValueError, match="SwingRacket-v0"):
        env.trace_step(None)
    assert stepper.trace_frame_substeps(776, 8, 98)[-1] == 776
