"""tb_sac_collect's C ABI and everything of the fused SAC / TQC collect that needs no GPU: the symbol is exported and a null handle is
refused by name, the ctypes mirror of TbSacCollectOut has the header's layout, plan_collect_chunks cuts a request where it must,
ReplayBuffer.reserve moves the cursor as add does, the scripts' flags reach the trainer, and the uniform mode's rule restated in
numpy (sac_collect_reference.uniform_actions, the GPU test's reference) is exact in float32."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_reference as pr
import sac_collect_reference as cr

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
    from tennisbot_rl_amd.stepper import TbSacCollectOut
    assert hasattr(lib, "tb_sac_collect")
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    out = TbSacCollectOut(ctypes.sizeof(TbSacCollectOut), p, p, p, p, p, None)
    assert lib.tb_sac_collect(None, p, 1, 0, 1, ctypes.byref(out), None) == -1   # TB_E_INVAL
    assert b"tb_sac_collect" in lib.tb_last_error()


def test_out_struct_layout_matches_the_header(tmp_path):
    """sizeof / offsetof from the C compiler == the ctypes mirror; the mode constants are the header's"""
    from tennisbot_rl_amd import stepper
    fields = [f[0] for f in stepper.TbSacCollectOut._fields_]
    assert fields == ["struct_size", "obs", "next_obs", "action", "reward", "done", "eps_or_null"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void){", 'printf("%zu\\n", sizeof(TbSacCollectOut));']
    prog += ['printf("%%zu\\n", offsetof(TbSacCollectOut, %s));' % f for f in fields]
    prog += ['printf("%d\\n%d\\n%d\\n", TB_SAC_COLLECT_ACTOR, TB_SAC_COLLECT_UNIFORM, TB_ABI_VERSION);', "return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(stepper.TbSacCollectOut)
    for f, off in zip(fields, out[1:]):
        assert getattr(stepper.TbSacCollectOut, f).offset == off, f
    assert out[-3:] == [stepper.SAC_COLLECT_ACTOR, stepper.SAC_COLLECT_UNIFORM, 4]   # the ABI version stays 4


# ------------------------------------------------------------------------------------------------------------ plan_collect_chunks
HAND_WORKED = [  # pos, capacity (vector steps), n_steps, SwingRacket phase or None, steps to learning_starts -> the launches
    ((0, 100, 1, None, 0), [1]),
    ((0, 100, 1, 25, 1), [1]),
    ((0, 100, 64, None, 0), [64]),
    ((2, 3, 1, None, 0), [1]),                 # the cursor at the ring's last row: one step fits ...
    ((2, 3, 2, None, 0), [1, 1]),              # ... and the second one starts the next lap
    ((2, 3, 5, None, 0), [1, 3, 1]),
    ((0, 100, 26, 0, 0), [26]),                # one whole SwingRacket episode
    ((0, 100, 27, 0, 0), [26, 1]),
    ((0, 100, 2, 25, 0), [1, 1]),              # phase 25: the next step ends the episodes
    ((0, 100, 30, 25, 0), [1, 26, 3]),
    ((0, 100, 8, None, 3), [3, 5]),            # learning_starts mid-request: three uniform steps, then the actor
    ((0, 100, 8, None, 8), [8]),
    ((0, 100, 8, None, 20), [8]),
    ((0, 100, 8, None, -5), [8]),              # long past
    ((0, 100, 8, None, None), [8]),
    ((0, 100, 40, 20, 8), [6, 2, 24, 8]),      # an episode end, then learning_starts, then the next episode end
    ((98, 100, 10, 24, 3), [2, 1, 7]),         # the wrap and the episode end together, then learning_starts
    ((97, 100, 6, None, 3), [3, 3]),           # the wrap and learning_starts at the same step: one cut
]


@pytest.mark.parametrize("args,want", HAND_WORKED)
def test_plan_collect_chunks_hand_worked(args, want):
    from tennisbot_rl_amd.sac import plan_collect_chunks
    assert plan_collect_chunks(*args) == want


def test_plan_collect_chunks_never_crosses_a_wrap_an_episode_end_or_learning_starts():
    from tennisbot_rl_amd.sac import plan_collect_chunks
    cases = 0
    for cap, S, phase, to_ls in itertools.product((1, 3, 26, 50), (1, 2, 7, 26, 27, 64, 130), (None, 0, 1, 13, 25), (None, -3, 0, 1, 5, 26, 1000)):
        for pos in sorted({0, cap // 2, cap - 1}):
            chunks = plan_collect_chunks(pos, cap, S, phase, to_ls)
            assert sum(chunks) == S and all(c >= 1 for c in chunks)
            p, ph, left_ls = pos, phase, (to_ls if to_ls is not None and to_ls > 0 else 0)
            for k, c in enumerate(chunks):
                assert p + c <= cap, "a launch crosses the wrap"
                at_cut = p + c == cap
                if ph is not None:
                    assert ph + c <= 26, "a launch crosses a SwingRacket episode end"
                    ph = (ph + c) % 26
                    at_cut |= ph == 0
                if left_ls > 0:
                    assert c <= left_ls, "a launch crosses the learning_starts step"
                    left_ls -= c
                    at_cut |= left_ls == 0
                assert at_cut or k == len(chunks) - 1, "a launch ended at none of the three cuts and not with the request"
                p = (p + c) % cap
            cases += 1
    assert cases > 1000
    assert plan_collect_chunks(0, 1, 1, None, 0) == [1]
    for bad in ((3, 3, 1, None, 0), (-1, 3, 1, None, 0), (0, 0, 1, None, 0), (0, 3, 0, None, 0), (0, 3, 1, 26, 0), (0, 3, 1, -1, 0)):
        with pytest.raises(ValueError):
            plan_collect_chunks(*bad)


# ------------------------------------------------------------------------------------------------------------ ReplayBuffer.reserve
def test_reserve_moves_the_cursor_as_add_does_and_its_views_alias_the_ring():
    import torch
    from tennisbot_rl_amd.sac import ReplayBuffer
    N, O, A, cap = 4, 3, 2, 24   # six vector steps
    a, b = ReplayBuffer(O, A, cap, "cpu"), ReplayBuffer(O, A, cap, "cpu")
    rng = np.random.default_rng(0)
    stamp, laps = 0.0, 0
    for steps in (1, 2, 3, 1, 5, 6, 2, 4, 1, 1, 3):   # every sequence member fits what is left of the lap or is cut at the wrap, as plan_collect_chunks would
        while steps:
            c = min(steps, (cap - a.pos) // N)
            steps -= c
            views = a.reserve(c, N)
            assert [tuple(v.shape) for v in views] == [(c * N, O), (c * N, O), (c * N, A), (c * N,), (c * N,)]
            rows = [torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32)) + stamp for v in views]
            stamp += 1.0
            for v, r in zip(views, rows):
                v.copy_(r)                      # written through the view ...
            b.add(*rows)                        # ... against add of the same rows
            assert (a.pos, a.size) == (b.pos, b.size)
            laps += a.pos == 0
            for x, y in zip(a.arrays(), b.arrays()):
                assert torch.equal(x, y)
            for v, arr in zip(views, a.arrays()):
                assert v.data_ptr() >= arr.data_ptr() and v.data_ptr() + v.numel() * 4 <= arr.data_ptr() + arr.numel() * 4 and v.is_contiguous()
    assert laps >= 3 and a.size == cap
    # refusals: a crossing reservation, a capacity or a cursor that is no multiple of n_envs, nothing moved by any of them
    pos, size = a.pos, a.size
    assert pos == 20                             # (29 vector steps into a ring of six: one step is left of this lap)
    with pytest.raises(ValueError, match="wrap"):
        a.reserve(2, N)
    with pytest.raises(ValueError, match="multiples"):
        ReplayBuffer(O, A, 25, "cpu").reserve(1, N)
    with pytest.raises(ValueError, match="multiples"):
        a.reserve(1, 8)                          # capacity 24 % 8 == 0, the cursor 20 % 8 != 0
    with pytest.raises(ValueError):
        a.reserve(0, N)
    assert (a.pos, a.size) == (pos, size)
    a.reserve(1, N)
    assert a.pos == 0


# ------------------------------------------------------------------------------------------------------------ scripts and trainer
@pytest.mark.parametrize("script", ["train_sac", "train_tqc"])
def test_collect_flags_parse_and_reach_the_trainer_arguments(script):
    import train_sac
    mod = __import__(script)
    parser = train_sac.off_policy_parser(*mod.PARSER)
    kw = train_sac.trainer_arguments(parser.parse_args([]))
    assert kw["collect_form"] == "torch" and kw["collect_steps"] == 1          # the defaults do not move
    assert kw["eval_form"] == "torch" and kw["num_envs"] == 256 and kw["gradient_steps"] is None and kw["learning_starts"] == 100
    args = parser.parse_args(["--collect-form", "fused", "--collect-steps", "8", "--gradient-steps", "4"])
    kw = train_sac.trainer_arguments(args)
    assert (kw["collect_form"], kw["collect_steps"], kw["gradient_steps"]) == ("fused", 8, 4)
    with pytest.raises(SystemExit):
        parser.parse_args(["--collect-form", "triton"])


def test_trainer_refuses_an_unknown_collect_form():
    from tennisbot_rl_amd.sac import COLLECT_FORMS, SACTrainer
    from tennisbot_rl_amd.tqc import TQCTrainer
    assert COLLECT_FORMS == ("torch", "fused")
    for trainer in (SACTrainer, TQCTrainer):
        with pytest.raises(ValueError, match="collect_form"):
            trainer("Tennisbot-v0", num_envs=16, collect_form="eager")
        with pytest.raises(ValueError, match="collect_steps"):
            trainer("Tennisbot-v0", num_envs=16, collect_form="fused", collect_steps=0)


# ------------------------------------------------------------------------------------------------------------ the uniform rule
def test_uniform_rule_is_exact_in_float32_and_stays_in_range():
    """float64 arithmetic on the same Philox words gives the same values: nothing was rounded; the words are policy_noise's"""
    seed = 0x5EED1234ABCD
    ids = (1 << 33) + np.arange(64, dtype=np.uint64)[None, :, None]
    ep = np.arange(3, dtype=np.uint64)[:, None, None]
    st = np.arange(40, dtype=np.int64)[None, None, :]
    for n_act in (2, 6):
        a = cr.uniform_actions(seed, ids, ep, st, n_act)
        assert a.dtype == np.float32 and a.shape == (3, 64, 40, n_act)
        key = (seed & pr.M32, (seed >> 32) ^ pr.NOISE_KEY_TAG)
        want = np.empty(a.shape, np.float64)
        for (e, i, s) in itertools.product(range(3), range(0, 64, 21), range(0, 40, 13)):
            words = []
            for blk in range((n_act + 3) // 4):
                eid = (1 << 33) + i
                words += list(pr.philox4x32((eid & pr.M32, eid >> 32, e, 4 * s + blk), key))
            want[e, i, s] = [(w >> 8) / 2.0 ** 23 - 1.0 for w in words[:n_act]]          # exact rationals in float64
            assert np.array_equal(a[e, i, s].astype(np.float64), want[e, i, s])
        assert a.min() >= -1.0 and a.max() <= 1.0 - 2.0 ** -23 and a.max() < 1.0
        assert np.array_equal(a * np.float32(2.0 ** 23), np.round(a * np.float32(2.0 ** 23)))   # multiples of 2^-23
        assert abs(float(a.mean())) < 0.02 and a.min() < -0.99 and a.max() > 0.99                # it does fill [-1, 1)
        assert len(np.unique(a[..., 0])) > 0.99 * a[..., 0].size                                 # keyed by env, episode and step
    # the range's ends come out of the extreme words
    assert np.float32(0) * np.float32(2.0 ** -23) - np.float32(1) == -1.0
    assert np.float32(2 ** 24 - 1) * np.float32(2.0 ** -23) - np.float32(1) == np.float32(1.0 - 2.0 ** -23)
