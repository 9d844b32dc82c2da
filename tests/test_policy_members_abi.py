"""tb_policy_evaluate_members' C ABI without a GPU: both symbols are exported, the granule is the tower wave's 16 envs, a null
handle is refused by name, and the ABI version did not move (the symbols are additive)."""
import ctypes
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


def test_symbols_are_exported_and_the_granule_is_the_tower_waves_slice(lib):
    assert hasattr(lib, "tb_policy_member_granule") and hasattr(lib, "tb_policy_evaluate_members")
    assert lib.tb_policy_member_granule() == 16
    assert lib.tb_abi_version() == 4


def test_a_null_handle_is_refused_by_name(lib):
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tb_policy_evaluate_members(None, 0, p, 1, 16, 16, p, p, 1, 0, None) == -1   # TB_E_INVAL
    assert b"tb_policy_evaluate_members" in lib.tb_last_error()


def test_the_python_side_granule_is_the_librarys(lib):
    from tennisbot_rl_amd import policy_es
    assert policy_es.MEMBER_GRANULE == lib.tb_policy_member_granule()
