"""tb_sac_evaluate_members' C ABI without a GPU: the symbol is exported beside an unchanged ABI version, a null handle is refused by
the entry point's name, and the Python method exists with the signature the tools call."""
import ctypes
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return load_library()


def test_symbol_is_exported_and_the_abi_version_did_not_move(lib):
    assert hasattr(lib, "tb_sac_evaluate_members")
    assert lib.tb_abi_version() == 4   # (the symbol is additive)


def test_a_null_handle_is_refused_by_name(lib):
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tb_sac_evaluate_members(None, p, 1, 70668, 16, p, p, 1, 0, None, None) == -1   # TB_E_INVAL
    assert b"tb_sac_evaluate_members" in lib.tb_last_error()


def test_python_method_signature():
    from tennisbot_rl_amd.stepper import BatchedEnv
    names = list(inspect.signature(BatchedEnv.sac_evaluate_members).parameters)
    assert names == ["self", "actors", "envs_per_member", "seed", "deterministic", "trace", "max_steps"]
