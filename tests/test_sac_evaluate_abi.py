"""tb_sac_evaluate's C ABI and the scripts' --eval-form, without a GPU: the symbol is exported, a null handle is refused by name,
the ctypes mirror of TbSacEvalTrace has the header's layout, and `--eval-form fused` reaches the trainer's arguments."""
import ctypes
import os
import subprocess
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


def test_symbol_is_exported_and_a_null_handle_is_refused_by_name(lib):
    assert hasattr(lib, "tb_sac_evaluate")
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.tb_sac_evaluate(None, p, p, p, 1, 0, None, None) == -1   # TB_E_INVAL
    assert b"tb_sac_evaluate" in lib.tb_last_error()


def test_trace_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof from the C compiler == the ctypes mirror"""
    from tennisbot_rl_amd.stepper import TbSacEvalTrace
    fields = [f[0] for f in TbSacEvalTrace._fields_]
    assert fields == ["struct_size", "max_steps", "obs", "eps", "actions", "reward", "done"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){", 'printf("%zu\\n", sizeof(TbSacEvalTrace));']
    prog += ['printf("%%zu\\n", offsetof(TbSacEvalTrace, %s));' % f for f in fields]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(TbSacEvalTrace)
    for f, off in zip(fields, out[1:]):
        assert getattr(TbSacEvalTrace, f).offset == off, f


@pytest.mark.parametrize("script", ["train_sac", "train_tqc"])
def test_eval_form_parses_and_reaches_the_trainer_argument(script):
    import train_sac
    mod = __import__(script)
    parser = train_sac.off_policy_parser(*mod.PARSER)
    assert train_sac.trainer_arguments(parser.parse_args([]))["eval_form"] == "torch"       # the default does not move
    args = parser.parse_args(["--eval-form", "fused", "--eval-freq", "1000"])
    assert args.eval_form == "fused" and train_sac.trainer_arguments(args)["eval_form"] == "fused"
    with pytest.raises(SystemExit):
        parser.parse_args(["--eval-form", "triton"])


def test_validate_takes_sac_and_tqc_and_asks_for_the_env():
    tool = os.path.join(ROOT, "tools", "validate.py")
    out = subprocess.run([sys.executable, tool, "-s", "sac", "-m", "nowhere.pt"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--env" in out.stderr
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tqc" in out.stdout and "--env" in out.stdout


def test_trainer_refuses_an_unknown_eval_form():
    from tennisbot_rl_amd.sac import EVAL_FORMS, SACTrainer
    assert EVAL_FORMS == ("torch", "fused")
    with pytest.raises(ValueError, match="eval_form"):
        SACTrainer("Tennisbot-v0", num_envs=16, eval_form="eager")
