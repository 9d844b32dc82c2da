"""What of the whole-episode evaluation needs no GPU: EvalSchedule's firing, best-model and checkpoint rules against a scripted
stub trainer (the counterpart of the reference's EvalCallback / CheckpointCallback, train_swing.py:111-119), `--load best`, and
the C ABI's new symbol (declared, exported, refusing null arguments before anything touches a device)."""
import ctypes
import os
import re

import pytest

from tennisbot_rl_amd.evaluation import BEST_MODEL, EvalSchedule, model_dir, resolve_load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tb_stepper.h")


class StubTrainer:
    """num_timesteps and mean returns are scripted; save() writes the timestep it was called at"""

    def __init__(self, means, rank=0):
        self.num_timesteps, self.rank = 0, rank
        self.means = list(means)
        self.eval_calls, self.saved = [], []

    def evaluate_episodes(self, n_episodes=64, deterministic=False):
        self.eval_calls.append((self.num_timesteps, n_episodes, deterministic))
        m = self.means.pop(0)
        return {"episodes": n_episodes, "mean": m, "std": 0.5, "min": m - 1.0, "max": m + 1.0, "mean_length": 26.0}

    def save(self, path):
        self.saved.append((self.num_timesteps, path))
        with open(path, "w") as fh:
            fh.write(str(self.num_timesteps))


def drive(schedule, trainer, timesteps):
    out = []
    for t in timesteps:
        trainer.num_timesteps = t
        out.append(schedule.after_rollout(trainer))
    return out


def test_one_evaluation_per_crossing_even_when_a_rollout_crosses_three_multiples(tmp_path):
    tr = StubTrainer([1.0, 2.0, 3.0, 4.0])
    s = EvalSchedule(eval_freq=1000, n_eval_episodes=7, deterministic=True, best_model_save_path=str(tmp_path))
    # 400, 900: below the first multiple; 1000: reaches it; 1100: no new one; 4300: crosses 2000, 3000 and 4000 at once -> ONE;
    # 4999: none; 5000: one
    got = drive(s, tr, [400, 900, 1000, 1100, 4300, 4999, 5000])
    assert [g is not None for g in got] == [False, False, True, False, True, False, True]
    assert tr.eval_calls == [(1000, 7, True), (4300, 7, True), (5000, 7, True)]
    assert s.history == [{"timesteps": t, "mean": m, "std": 0.5, "mean_length": 26.0, "episodes": 7} for t, m in ((1000, 1.0), (4300, 2.0), (5000, 3.0))]


def test_best_model_is_written_only_on_strict_improvement(tmp_path):
    tr = StubTrainer([5.0, 5.0, 4.0, 6.0, -1.0])
    s = EvalSchedule(eval_freq=10, best_model_save_path=str(tmp_path / "m"))
    drive(s, tr, [10, 20, 30, 40, 50])
    best = os.path.join(str(tmp_path / "m"), "best_model.pt")
    assert s.best_model_path() == best and BEST_MODEL == "best_model.pt"
    assert tr.saved == [(10, best), (40, best)]          # 5 (the first), then only 6: an equal mean and worse ones keep the file
    assert open(best).read() == "40" and s.best_mean == 6.0
    assert len(s.history) == 5
    # a negative first mean is an improvement over "nothing yet"
    tr2 = StubTrainer([-30.0])
    s2 = EvalSchedule(eval_freq=10, best_model_save_path=str(tmp_path / "n"))
    drive(s2, tr2, [10])
    assert [t for t, _ in tr2.saved] == [10]
    # without a path the best is tracked and nothing is written
    tr3 = StubTrainer([1.0, 2.0])
    s3 = EvalSchedule(eval_freq=10)
    drive(s3, tr3, [10, 20])
    assert tr3.saved == [] and s3.best_mean == 2.0 and s3.best_model_path() is None


def test_checkpoints_are_named_after_the_timesteps_they_were_taken_at(tmp_path):
    tr = StubTrainer([])
    s = EvalSchedule(save_freq=10000, save_path=str(tmp_path), name_prefix="rl_model")
    drive(s, tr, [4096, 8192, 12288, 16384, 20480, 53248])
    names = [os.path.basename(p) for _, p in tr.saved]
    assert names == ["rl_model_12288_steps.pt", "rl_model_20480_steps.pt", "rl_model_53248_steps.pt"]   # 53248 crossed 30000, 40000, 50000: one file
    assert s.checkpoints == [p for _, p in tr.saved] and all(os.path.exists(p) for p in s.checkpoints)
    assert tr.eval_calls == [] and s.history == []      # eval_freq = 0: no evaluation
    s2 = EvalSchedule(save_freq=5, save_path=str(tmp_path), name_prefix="tuned")
    assert os.path.basename(s2.checkpoint_path(15)) == "tuned_15_steps.pt"
    with pytest.raises(ValueError):
        EvalSchedule(save_freq=5)


def test_both_frequencies_and_a_resumed_count(tmp_path):
    tr = StubTrainer([1.0, 0.0])
    s = EvalSchedule(eval_freq=100, save_freq=250, best_model_save_path=str(tmp_path), save_path=str(tmp_path))
    s.reset(1000)                       # a resumed run: the multiples below 1000 are behind it
    drive(s, tr, [1040, 1100, 1260])
    assert [t for t, _, _ in tr.eval_calls] == [1100, 1260]
    assert [(t, os.path.basename(p)) for t, p in tr.saved] == [(1100, "best_model.pt"), (1260, "rl_model_1260_steps.pt")]


def test_other_ranks_neither_evaluate_nor_write(tmp_path):
    tr = StubTrainer([1.0, 2.0], rank=1)
    s = EvalSchedule(eval_freq=10, save_freq=10, best_model_save_path=str(tmp_path), save_path=str(tmp_path))
    assert drive(s, tr, [10, 20, 30]) == [None, None, None]
    assert tr.eval_calls == [] and tr.saved == [] and s.history == [] and s.checkpoints == [] and os.listdir(str(tmp_path)) == []


def test_schedule_draws_nothing_from_the_torch_rng(tmp_path):
    import torch
    torch.manual_seed(3)
    before = torch.get_rng_state().clone()
    drive(EvalSchedule(eval_freq=10, save_freq=10, best_model_save_path=str(tmp_path), save_path=str(tmp_path)), StubTrainer([1.0, 2.0]), [10, 20])
    assert torch.equal(torch.get_rng_state(), before)


def test_load_best_resolves_beside_the_save_path(tmp_path):
    save = os.path.join(str(tmp_path), "model", "tuned_ppo_Tennisbot-v0.pt")
    assert resolve_load("best", save) == os.path.join(str(tmp_path), "model", "best_model.pt")
    assert resolve_load("best", "x.pt") == os.path.join(os.getcwd(), "best_model.pt")
    assert resolve_load("elsewhere/ck.pt", save) == "elsewhere/ck.pt" and resolve_load(None, save) is None
    assert model_dir(save) == os.path.join(str(tmp_path), "model")
    # the scripts' schedule writes where --load best reads
    import argparse
    from tennisbot_rl_amd.evaluation import add_schedule_arguments, schedule_from_args
    ap = argparse.ArgumentParser()
    add_schedule_arguments(ap)
    assert schedule_from_args(ap.parse_args([]), save) is None                       # every flag off: today's behaviour
    s = schedule_from_args(ap.parse_args(["--eval-freq", "2e5", "--save-freq", "1e6", "--n-eval-episodes", "32"]), save, log=None)
    assert s.best_model_path() == resolve_load("best", save) and (s.eval_freq, s.save_freq, s.n_eval_episodes, s.deterministic) == (200000, 1000000, 32, False)
    assert s.checkpoint_path(1003520) == os.path.join(str(tmp_path), "model", "rl_model_1003520_steps.pt")


# ------------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    from tennisbot_rl_amd.build import build_library
    from tennisbot_rl_amd.stepper import load_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return load_library()


def test_header_declares_and_library_exports_tb_policy_evaluate(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+tb_policy_evaluate\s*\(([^)]*)\)\s*;", src)
    assert m, "include/tb_stepper.h does not declare tb_policy_evaluate"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["TbHandle *h", "int net", "const float *weights_dev", "double *return_dev", "int32_t *length_dev", "uint64_t noise_seed",
                    "int deterministic", "void *stream"]
    assert hasattr(lib, "tb_policy_evaluate")
    assert lib.tb_abi_version() == 4          # an additive symbol
    assert lib.tb_policy_evaluate.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.c_int, ctypes.c_void_p]


def test_null_handle_and_null_buffers_are_refused_with_a_message(lib):
    buf = (ctypes.c_double * 4)()
    p = ctypes.addressof(buf)
    fake = ctypes.addressof((ctypes.c_char * 64)())   # never dereferenced: every null check comes first
    for h, w, r, ln in ((None, p, p, p), (fake, None, p, p), (fake, p, None, p), (fake, p, p, None), (None, None, None, None)):
        assert lib.tb_policy_evaluate(h, 0, w, r, ln, 1, 0, None) == -1   # TB_E_INVAL
        msg = lib.tb_last_error()
        assert b"tb_policy_evaluate" in msg and b"null" in msg, msg
