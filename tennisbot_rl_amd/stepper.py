"""Tensor API over the C ABI (include/tb_stepper.h): N independent (racket, ball) worlds
stepped in lockstep on one MI355X.

This is the measured path: `step(actions)` takes and returns device tensors and never
synchronises with the host. torch is used for device memory and streams only; all
arithmetic happens in libtb_stepper.so (hand-written HIP: csrc/tb_kernels.hpp, tb_device.hpp, tb_policy.hpp, tb_render.hpp, tb_trace.hpp; host side csrc/tb_stepper.hip). There is
no CPU or eager-PyTorch fallback: if the library or a GPU is missing, construction raises.

Reference counterparts: `SwingRacketEnv` (tennisbot/envs/swingracket_env.py:24-192) and
`TennisbotEnv` (tennisbot/envs/tennisbot_env.py:27-291), one PyBullet world each.
"""
import ctypes
import os

import numpy as np

from .params import (ACT_DIM, COUNTER_NAMES, ENV_SWING, ENV_TENNIS, F_AUTO_RESET, N_COUNTERS, NET_DEFAULT, NET_MLP64, NET_TUNED, OBS_DIM,  # noqa: F401
                     STATE_ROWS, STATE_WORDS, TbOptions, TbParams, default_params, make_options)

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtb_stepper.so")
_LIB = None
ABI_VERSION = 4

ENV_IDS = {"SwingRacket-v0": ENV_SWING, "Tennisbot-v0": ENV_TENNIS}  # tennisbot/__init__.py:3-11


class StepperError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def use_library(path):
    """Load another BUILD of the same sources instead of the in-tree one (the -DTB_DIAG_* diagnostic builds of
    tools/diag_*.py). An explicit call before the first BatchedEnv, not an environment variable: nothing
    outside the caller's own code can redirect the product path."""
    global _LIB_PATH, _LIB
    if _LIB is not None:
        raise StepperError("use_library() must be called before the library is first loaded")
    _LIB_PATH = os.path.abspath(path)


def load_library():
    """dlopen the HIP library. Fails loudly: the product has no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise StepperError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % _LIB_PATH)
    # torch first: the library must run on torch's HIP runtime, whose device memory and streams it is handed. torch's own
    # libraries ask for "libamdhip64.so" by that name; loaded after ours, they would map a second HIP (and HSA) runtime into
    # the process, and one of the two then finds no device. Loaded before, our "libamdhip64.so.7" resolves to torch's copy.
    import torch  # noqa: F401
    L = ctypes.CDLL(_LIB_PATH)
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    L.tb_abi_version.restype = i32
    L.tb_obs_dim.argtypes = [i32]
    L.tb_act_dim.argtypes = [i32]
    L.tb_state_words.argtypes = [i32]
    L.tb_last_error.restype = ctypes.c_char_p
    L.tb_create.argtypes = [ctypes.POINTER(TbParams), ctypes.POINTER(TbOptions), i32, i32, i32, u64, u64, ctypes.POINTER(vp)]
    L.tb_destroy.argtypes = [vp]
    L.tb_set_params.argtypes = [vp, ctypes.POINTER(TbParams), vp]
    L.tb_reset.argtypes = [vp, vp, vp, vp]
    L.tb_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.tb_rollout.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.tb_get_state.argtypes = [vp, vp, vp, i32, vp]
    L.tb_set_state.argtypes = [vp, vp, vp, i32, vp]
    L.tb_counters.argtypes = [vp, vp, vp]
    L.tb_counters_reset.argtypes = [vp, vp]
    L.tb_sealed_substeps.argtypes = [vp, vp, vp]
    L.tb_set_pipeline.argtypes = [vp, i32]
    L.tb_set_pipeline.restype = i32
    L.tb_flush.argtypes = [vp, vp]
    L.tb_flush.restype = i32
    L.tb_pipeline_sync.argtypes = [vp, i32]
    L.tb_pipeline_sync.restype = i32
    L.tb_policy_rollout.argtypes = [vp, i32] + [vp] * 9 + [ctypes.POINTER(ctypes.c_size_t), u64, i32, vp]
    L.tb_policy_rollout.restype = i32
    L.tb_step_sequence.argtypes = [vp, i32, vp, vp, vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]
    L.tb_step_sequence.restype = i32
    L.tb_policy_floats.argtypes = [i32]
    L.tb_policy_floats.restype = i32
    L.tb_policy_step.argtypes = [vp] * 10 + [u64, i32, vp]
    L.tb_policy_step.restype = i32
    L.tb_policy_blob_floats.argtypes = [i32, i32]
    L.tb_policy_blob_floats.restype = i32
    L.tb_policy_step_net.argtypes = [vp, i32] + [vp] * 9 + [u64, i32, vp]
    L.tb_policy_step_net.restype = i32
    L.tb_policy_rollout_net.argtypes = [vp, i32, i32] + [vp] * 9 + [ctypes.POINTER(ctypes.c_size_t), u64, i32, vp]
    L.tb_policy_rollout_net.restype = i32
    L.tb_es_floats.argtypes = [i32]
    L.tb_es_floats.restype = i32
    L.tb_es_evaluate.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, vp, vp, ctypes.POINTER(TbEsTrace), vp]
    L.tb_es_evaluate.restype = i32
    L.tb_policy_evaluate.argtypes = [vp, i32, vp, vp, vp, u64, i32, vp]
    L.tb_policy_evaluate.restype = i32
    L.tb_policy_member_granule.argtypes = []
    L.tb_policy_member_granule.restype = i32
    L.tb_policy_evaluate_members.argtypes = [vp, i32, vp, i32, ctypes.c_size_t, i32, vp, vp, u64, i32, vp]
    L.tb_policy_evaluate_members.restype = i32
    L.tb_policy_rollout_members.argtypes = [vp, i32, i32, vp, i32, ctypes.c_size_t, i32] + [vp] * 8 + [ctypes.POINTER(ctypes.c_size_t), u64, i32, vp]
    L.tb_policy_rollout_members.restype = i32
    L.tb_sac_evaluate.argtypes = [vp, vp, vp, vp, u64, i32, ctypes.POINTER(TbSacEvalTrace), vp]
    L.tb_sac_evaluate.restype = i32
    L.tb_sac_evaluate_members.argtypes = [vp, vp, i32, ctypes.c_size_t, i32, vp, vp, u64, i32, ctypes.POINTER(TbSacEvalTrace), vp]
    L.tb_sac_evaluate_members.restype = i32
    L.tb_sac_collect.argtypes = [vp, vp, i32, i32, u64, ctypes.POINTER(TbSacCollectOut), vp]
    L.tb_sac_collect.restype = i32
    f32, f64, i64 = ctypes.c_float, ctypes.c_double, ctypes.c_longlong
    L.tb_ppo_param_floats.argtypes = [i32]
    L.tb_ppo_param_floats.restype = i32
    L.tb_ppo_rows_per_workgroup.argtypes = []
    L.tb_ppo_rows_per_workgroup.restype = i32
    L.tb_ppo_workspace_bytes.argtypes = [i32, i32]
    L.tb_ppo_workspace_bytes.restype = i64
    L.tb_ppo_gae.argtypes = [i32, i32, vp, i32, i32, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp, f64, f64, vp, vp]
    L.tb_ppo_gae.restype = i32
    L.tb_ppo_grad.argtypes = [i32, i32, vp] + [vp] * 5 + [i64, vp, i32, vp, i32, f32, f32, vp, ctypes.c_size_t]
    L.tb_ppo_grad.restype = i32
    L.tb_ppo_apply.argtypes = [i32, i32, vp, i32, vp, ctypes.c_size_t, i32] + [vp] * 4 + [i32, vp, f32, f32, i32, f32, f32, f32, f32, i64]
    L.tb_ppo_apply.restype = i32
    L.tb_ppo_param_floats_net.argtypes = [i32, i32]
    L.tb_ppo_param_floats_net.restype = i32
    L.tb_ppo_workspace_bytes_net.argtypes = [i32, i32, i32]
    L.tb_ppo_workspace_bytes_net.restype = i64
    L.tb_ppo_grad_net.argtypes = [i32, i32, i32, vp] + [vp] * 5 + [i64, vp, i32, vp, i32, f32, f32, vp, ctypes.c_size_t]
    L.tb_ppo_grad_net.restype = i32
    L.tb_ppo_apply_net.argtypes = [i32, i32, i32, vp, i32, vp, ctypes.c_size_t, i32] + [vp] * 4 + [i32, vp, f32, f32, i32, f32, f32, f32, f32, i64]
    L.tb_ppo_apply_net.restype = i32
    L.tb_ppo_members_workspace_stride_bytes.argtypes = [i32, i32, i32]
    L.tb_ppo_members_workspace_stride_bytes.restype = i64
    L.tb_ppo_grad_members.argtypes = [i32, i32, i32, vp] + [vp] * 5 + [i64, vp, ctypes.c_size_t, i32, i32, vp, ctypes.c_size_t, i32, vp, vp, ctypes.c_size_t]
    L.tb_ppo_grad_members.restype = i32
    L.tb_ppo_apply_members.argtypes = [i32, i32, i32, vp, vp, ctypes.c_size_t, i32, i32] + [vp] * 4 + [ctypes.c_size_t, i32, vp, vp, f32, f32, f32, f32, i64]
    L.tb_ppo_apply_members.restype = i32
    L.tb_trpo_rows_per_workgroup.argtypes = []
    L.tb_trpo_rows_per_workgroup.restype = i32
    L.tb_trpo_search_rows_per_workgroup.argtypes = []
    L.tb_trpo_search_rows_per_workgroup.restype = i32
    L.tb_trpo_fvp_workspace_bytes.argtypes = [i32, i32]
    L.tb_trpo_fvp_workspace_bytes.restype = i64
    L.tb_trpo_search_workspace_bytes.argtypes = [i32, i32, i32]
    L.tb_trpo_search_workspace_bytes.restype = i64
    L.tb_trpo_fvp.argtypes = [i32, i32, vp, vp, i64, vp, i32, vp, vp, i32, f32, vp, vp, ctypes.c_size_t]
    L.tb_trpo_fvp.restype = i32
    L.tb_trpo_search.argtypes = [i32, i32, vp] + [vp] * 4 + [i64, vp, i32, vp, vp, i32, vp, i32, vp, vp, ctypes.c_size_t]
    L.tb_trpo_search.restype = i32
    L.tb_trpo_fvp_workspace_bytes_net.argtypes = [i32, i32, i32]
    L.tb_trpo_fvp_workspace_bytes_net.restype = i64
    L.tb_trpo_search_workspace_bytes_net.argtypes = [i32, i32, i32, i32]
    L.tb_trpo_search_workspace_bytes_net.restype = i64
    L.tb_trpo_fvp_net.argtypes = [i32, i32, i32, vp, vp, i64, vp, i32, vp, vp, i32, f32, vp, vp, ctypes.c_size_t]
    L.tb_trpo_fvp_net.restype = i32
    L.tb_trpo_search_net.argtypes = [i32, i32, i32, vp] + [vp] * 4 + [i64, vp, i32, vp, vp, i32, vp, i32, vp, vp, ctypes.c_size_t]
    L.tb_trpo_search_net.restype = i32
    L.tb_trpo_returns_workspace_bytes.argtypes = [i32, i32]
    L.tb_trpo_returns_workspace_bytes.restype = i64
    L.tb_trpo_returns.argtypes = [i32, i32, vp, i32, i32, vp, ctypes.c_size_t, vp, ctypes.c_size_t, f64, vp, vp, vp, vp, ctypes.c_size_t]
    L.tb_trpo_returns.restype = i32
    L.tb_sac_param_floats.argtypes = [i32, i32]
    L.tb_sac_param_floats.restype = i32
    L.tb_sac_rows_per_workgroup.argtypes = []
    L.tb_sac_rows_per_workgroup.restype = i32
    L.tb_sac_workspace_bytes.argtypes = [i32, i32]
    L.tb_sac_workspace_bytes.restype = i64
    L.tb_sac_actor_forward.argtypes = [i32, i32, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.tb_sac_actor_forward.restype = i32
    L.tb_sac_targets.argtypes = [i32, i32, vp, vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, f32, vp, vp, ctypes.c_size_t]
    L.tb_sac_targets.restype = i32
    L.tb_sac_critic_grad.argtypes = [i32, i32, vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.tb_sac_critic_grad.restype = i32
    L.tb_sac_actor_grad.argtypes = [i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    L.tb_sac_actor_grad.restype = i32
    L.tb_sac_adam.argtypes = [i32, vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, vp, f32]
    L.tb_sac_adam.restype = i32
    L.tb_tqc_param_floats.argtypes = [i32, i32]
    L.tb_tqc_param_floats.restype = i32
    L.tb_tqc_workspace_bytes.argtypes = [i32, i32]
    L.tb_tqc_workspace_bytes.restype = i64
    for sac, tqc in ((L.tb_sac_actor_forward, L.tb_tqc_actor_forward), (L.tb_sac_targets, L.tb_tqc_targets), (L.tb_sac_critic_grad, L.tb_tqc_critic_grad),
                     (L.tb_sac_actor_grad, L.tb_tqc_actor_grad)):   # the same signatures
        tqc.argtypes, tqc.restype = sac.argtypes, i32
    sz = ctypes.c_size_t
    members = {"members_workspace_stride_bytes": ([i32, i32], i64),
               "actor_forward_members": ([i32, i32, vp, vp, i64, vp, sz, i32, i32, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz], i32),
               "targets_members": ([i32, i32, vp, vp, vp, vp, i64, vp, sz, i32, i32, vp, sz, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz], i32),
               "critic_grad_members": ([i32, i32, vp, vp, vp, i64, vp, sz, i32, i32, vp, sz, vp, sz, vp, vp, vp, sz], i32),
               "actor_grad_members": ([i32, i32, vp, i32, i32, vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, sz], i32)}
    for prefix in ("tb_sac_", "tb_tqc_"):   # the same signatures
        for name, (argtypes, restype) in members.items():
            f = getattr(L, prefix + name)
            f.argtypes, f.restype = argtypes, restype
    L.tb_sac_adam_members.argtypes = [i32, vp, vp, vp, vp, vp, i64, sz, i32, vp, i32, f32, f32, f32, i64, vp]
    L.tb_sac_adam_members.restype = i32
    L.tb_render.argtypes = [i32, i32, vp, ctypes.POINTER(TbParams), vp, i32, vp, i32, ctypes.POINTER(TbCamera), i32, i32, vp, vp, vp]
    L.tb_render.restype = i32
    L.tb_swing_trace.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tb_swing_trace.restype = i32
    L.tb_phase.argtypes = [vp]
    L.tb_phase.restype = i32
    L.tb_phase_advance.argtypes = [vp, i32]
    L.tb_phase_advance.restype = i32
    L.tb_pipeline_form.argtypes = [vp]
    L.tb_pipeline_form.restype = i32
    L.tb_step_waves.argtypes = [vp]
    L.tb_step_waves.restype = i32
    L.tb_step_form.argtypes = [vp]
    L.tb_step_form.restype = i32
    L.tb_params_generation.argtypes = [vp]
    L.tb_params_generation.restype = i32
    L.tb_set_racket_scale.argtypes = [vp, ctypes.c_float, vp]
    L.tb_set_racket_scale.restype = i32
    L.tb_pipeline_recover.argtypes = [vp]
    L.tb_pipeline_recover.restype = i32
    L.tb_mark_record.argtypes = [vp, i32, vp]
    L.tb_mark_record.restype = i32
    L.tb_mark_count.argtypes = [vp, i32]
    L.tb_mark_count.restype = ctypes.c_longlong
    L.tb_mark_host_wait.argtypes = [vp, i32, i32]
    L.tb_mark_host_wait.restype = i32
    L.tb_mark_begin.argtypes = [vp]
    L.tb_mark_begin.restype = i32
    L.tb_mark_enable.argtypes = [vp, i32]
    L.tb_mark_enable.restype = i32
    L.tb_diag_stream_copy.argtypes = [vp, vp, i32, i32, i32, vp]
    L.tb_diag_stream_copy.restype = i32
    L.tb_diag_idle.argtypes = [i32, i32, i32, vp]
    L.tb_diag_idle.restype = i32
    L.tb_diag_two_wave_gate.argtypes = [vp, vp, vp]
    L.tb_diag_two_wave_gate.restype = i32
    L.tb_diag_fail_alloc.argtypes = [i32]
    L.tb_diag_fail_alloc.restype = i32
    for f in ("tb_create", "tb_destroy", "tb_set_params", "tb_reset", "tb_step", "tb_rollout", "tb_get_state",
              "tb_set_state", "tb_counters", "tb_counters_reset", "tb_obs_dim", "tb_act_dim", "tb_state_words"):
        getattr(L, f).restype = i32
    if L.tb_abi_version() != ABI_VERSION:
        raise StepperError("libtb_stepper.so ABI version %d, expected %d" % (L.tb_abi_version(), ABI_VERSION))
    for kind in (ENV_SWING, ENV_TENNIS):
        assert L.tb_obs_dim(kind) == OBS_DIM[kind] and L.tb_act_dim(kind) == ACT_DIM[kind]
        assert L.tb_state_words(kind) == STATE_WORDS[kind]
    _LIB = L
    return L


class TbEsTrace(ctypes.Structure):
    """include/tb_stepper.h TbEsTrace: optional per-step record of tb_es_evaluate"""
    _fields_ = [("struct_size", ctypes.c_size_t), ("max_steps", ctypes.c_int), ("net_in", ctypes.c_void_p), ("obs", ctypes.c_void_p),
                ("actions", ctypes.c_void_p), ("raw", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p)]


class TbSacEvalTrace(ctypes.Structure):
    """include/tb_stepper.h TbSacEvalTrace: optional per-step record of tb_sac_evaluate"""
    _fields_ = [("struct_size", ctypes.c_size_t), ("max_steps", ctypes.c_int), ("obs", ctypes.c_void_p), ("eps", ctypes.c_void_p),
                ("actions", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p)]


class TbSacCollectOut(ctypes.Structure):
    """include/tb_stepper.h TbSacCollectOut: the [S][N] rows tb_sac_collect writes (pointers into the caller's replay ring)"""
    _fields_ = [("struct_size", ctypes.c_size_t), ("obs", ctypes.c_void_p), ("next_obs", ctypes.c_void_p), ("action", ctypes.c_void_p),
                ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p), ("eps_or_null", ctypes.c_void_p)]


SAC_COLLECT_ACTOR, SAC_COLLECT_UNIFORM = 0, 1   # include/tb_stepper.h TB_SAC_COLLECT_*


class TbCamera(ctypes.Structure):
    """include/tb_stepper.h TbCamera: the view of tb_render"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("eye", ctypes.c_float * 3), ("target", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("fov_y_deg", ctypes.c_float), ("follow", ctypes.c_int32), ("light_dir", ctypes.c_float * 3)]


DEFAULT_LIGHT = (0.3, -0.5, 0.8)
RENDER_IDS = ("sky", "ground", "net", "goal", "ball", "racket")   # the id layer of tb_render


def Camera(eye, target, up=(0.0, 0.0, 1.0), fov_y_deg=60.0, follow=False, light_dir=DEFAULT_LIGHT):
    """A TbCamera. follow=True: eye and target are offsets from EACH env's racket COM. Bad values (eye == target, up parallel to the
    view, fov outside (0, 180)) are refused by the library when the camera is used."""
    c = TbCamera()
    c.struct_size = ctypes.sizeof(TbCamera)
    for i in range(3):
        c.eye[i], c.target[i], c.up[i], c.light_dir[i] = float(eye[i]), float(target[i]), float(up[i]), float(light_dir[i])
    c.fov_y_deg, c.follow = float(fov_y_deg), 1 if follow else 0
    return c


def default_camera(kind):
    """The view that shows what a policy does, for each env its own: a follow camera behind and above the env's racket, looking past it
    down the court towards the net (SwingRacket-v0: and the goal beyond it; Tennisbot-v0: towards the incoming ball). The rackets
    spawn anywhere in a 5 m x 8 m (10 m) region (swingracket_env.py:161-162, tennisbot_env.py:227-228), which no fixed camera
    shows at a readable size: court_camera() is that fixed overview."""
    if isinstance(kind, str):
        kind = ENV_IDS[kind]
    if kind == ENV_SWING:
        return Camera((3.5, -2.0, 2.2), (-3.0, 0.5, 0.2), follow=True)
    return Camera((3.0, -1.5, 1.5), (-2.0, 0.3, -0.2), follow=True)


def court_camera():
    """a fixed view of the whole court from beside the racket's end"""
    return Camera((20.0, -11.0, 8.0), (1.0, 0.0, 0.0))


def racket_view(racket_pos, racket_quat):
    """The camera the reference's render() builds (tennisbot_env.py:263-279): at the racket with z = 0.2, looking along the body x
    axis, the body z axis up, fov 80. It needs the orientation, so it is built per call from ONE env's state (get_state()'s
    racket_pos[i], racket_quat[i])."""
    x, y, z, w = (float(v) for v in racket_quat)
    ex = (1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w))   # R [1, 0, 0]
    ez = (2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y))   # R [0, 0, 1]
    eye = (float(racket_pos[0]), float(racket_pos[1]), 0.2)
    return Camera(eye, tuple(e + d for e, d in zip(eye, ex)), up=ez, fov_y_deg=80.0)


def render_words(kind, params, words, indices=None, camera=None, width=96, height=64, layers=False):
    """tb_render on a state-word block: words int32 / uint32 [W, N] on a GPU (get_state_words' layout) -> uint8 [K, H, W, 3] on the same
    device; with layers=True also ids uint8 [K, H, W] (RENDER_IDS) and depth float32 [K, H, W] (+inf: sky). indices: the envs to show (a
    sequence or an integer tensor; any order, repeats allowed, out-of-range values clamped), default all. Stream-ordered, no host sync."""
    import torch as t
    L = load_library()
    if isinstance(kind, str):
        kind = ENV_IDS[kind]
    if not isinstance(words, t.Tensor) or words.device.type != "cuda" or words.dim() != 2 or words.shape[0] != STATE_WORDS[kind] or not words.is_contiguous():
        raise ValueError("words must be a contiguous [%d, N] tensor on the GPU" % STATE_WORDS[kind])
    if words.element_size() != 4:
        raise TypeError("words must hold 32-bit words")
    n = int(words.shape[1])
    idx = None
    if indices is not None:
        idx = indices if isinstance(indices, t.Tensor) else t.as_tensor(np.asarray(indices, dtype=np.int64).reshape(-1))
        idx = idx.to(device=words.device, dtype=t.int32).contiguous()
    K = n if idx is None else int(idx.numel())
    cam = camera if camera is not None else default_camera(kind)
    W, H = int(width), int(height)
    shape = (K, max(H, 0), max(W, 0))   # a size < 1 is the library's to refuse
    rgb = t.empty(shape + (3,), dtype=t.uint8, device=words.device)
    ids = t.empty(shape, dtype=t.uint8, device=words.device) if layers else None
    depth = t.empty(shape, dtype=t.float32, device=words.device) if layers else None
    _check(L, L.tb_render(int(kind), words.device.index, ctypes.c_void_p(t.cuda.current_stream(words.device).cuda_stream), ctypes.byref(params),
                          words.data_ptr(), n, None if idx is None else idx.data_ptr(), K, ctypes.byref(cam), W, H, rgb.data_ptr(),
                          None if ids is None else ids.data_ptr(), None if depth is None else depth.data_ptr()), "tb_render")
    return (rgb, ids, depth) if layers else rgb


TRACE_MAX_SUBSTEPS = 776   # a SwingRacket-v0 step: the agent's substep + at most 775 of the fast-forward (swingracket_env.py:105-129)


def trace_frame_substeps(ns, stride, max_frames):
    """tb_swing_trace's sampling rule (include/tb_stepper.h) in plain Python: the substep numbers s, 1-based, of the max_frames stored
    rows of an env whose step ran ns substeps. The samples are 1, 1 + stride, 1 + 2 stride, ... <= ns, then ns itself; where they
    fit, the rows behind them repeat ns, and where they do not, the last row is ns all the same. n_frames reports how many samples
    there were: 1 + (ns - 1) // stride + ((ns - 1) % stride != 0), whether they fit or not."""
    ns, stride, F = int(ns), int(stride), int(max_frames)
    if ns < 1 or stride < 1 or F < 1:
        raise ValueError("ns, stride and max_frames must be >= 1")
    samples = list(range(1, ns + 1, stride))
    if samples[-1] != ns:
        samples.append(ns)
    if len(samples) <= F:
        return samples + [ns] * (F - len(samples))
    return samples[:F - 1] + [ns]


def _check(L, rc, what):
    if rc != 0:
        raise StepperError("%s failed (%d): %s" % (what, rc, L.tb_last_error().decode()))


def check_net(kind, net):
    """the library's refusal of (Tennisbot-v0, NET_MLP64) as a ValueError, before any call: that pair is not a missing kernel but
    another name for what NET_DEFAULT already is there"""
    if int(net) == NET_MLP64 and int(kind) == ENV_TENNIS:
        raise ValueError("NET_MLP64 is SwingRacket-v0's; on Tennisbot-v0 NET_DEFAULT (TB_NET_DEFAULT) is that net: pi = vf = [64, 64], tanh")
    return int(net)


class StepGraph:
    """K captured agent steps of one BatchedEnv (BatchedEnv.capture). replay() runs them with one launch --
    after checking what a captured launch cannot check for itself:
      * the parameter block travels in the kernel arguments, so a graph captured before set_params() would
        step with the old parameters: refused (recapture); set_racket_scale() is exempt, the kernels read
        the scale from device memory;
      * a pipelined SwingRacket graph bakes in WHICH of its steps end an episode (and fork a fast-forward):
        it is only valid from the episode phase it was captured at. K % 26 != 0, or steps taken outside the
        graph in between, move the phase: refused, instead of episode ends falling into launches that have
        no fast-forward slot (their terminal rewards would be lost, counters()['lockstep_violations'])."""

    def __init__(self, env, graph, n_steps, phase, generation):
        self.env, self.graph, self.n_steps, self.phase, self.generation = env, graph, int(n_steps), phase, generation

    @property
    def repeatable(self):
        return self.phase < 0 or self.n_steps % 26 == 0

    def valid(self):
        """may replay() run now? (same parameter block, same episode phase as at capture time)"""
        env = self.env
        return env.L.tb_params_generation(env._h) == self.generation and (self.phase < 0 or env.L.tb_phase(env._h) == self.phase)

    def replay(self):
        env = self.env
        if env.L.tb_params_generation(env._h) != self.generation:
            raise StepperError("this graph was captured before set_params(): its launches carry the old parameter block; capture it again")
        if self.phase >= 0:
            now = env.L.tb_phase(env._h)
            if now != self.phase:
                raise StepperError("this graph was captured at episode phase %d and can only be replayed from there; the envs are at phase %d "
                                   "(captured steps %% 26 = %d; or steps were taken outside the graph)" % (self.phase, now, self.n_steps % 26))
        if env.pipeline:
            # eager pipelined steps may still have fast-forwards running on the handle's side streams; the captured launches bake
            # in slot indices and hold no wait on them (the capture began with every slot idle). Up to 8 hipStreamWaitEvent
            # calls, nothing when no slot is busy.
            env.flush()
        self.graph.replay()
        _check(env.L, env.L.tb_phase_advance(env._h, self.n_steps), "tb_phase_advance")


class BatchedEnv:
    """N lockstep worlds of one env kind on one GPU.

    step(actions) -> (obs, reward, done): float32 [N, O], float32 [N], uint8 [N] device tensors.
    With auto_reset (default, SB3 VecEnv semantics) an env that finishes is reset inside the
    same kernel: `obs` then holds the first observation of the new episode and
    `terminal_obs()` the last one of the old episode. With auto_reset=False `done` is sticky
    until reset(), exactly like the reference's `self.done`.
    """

    def __init__(self, env_kind, num_envs, device=None, seed=0, env_id_base=0, params=None, auto_reset=True,
                 reuse_buffers=False, track_terminal_obs=True, pipeline=False, options=None):
        import torch
        self.torch = torch
        if isinstance(env_kind, str):
            env_kind = ENV_IDS[env_kind]
        if env_kind not in (ENV_SWING, ENV_TENNIS):
            raise ValueError("unknown env kind %r" % (env_kind,))
        self.L = load_library()
        if not torch.cuda.is_available():
            raise StepperError("no GPU visible to torch: the batched stepper is HIP-only (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise StepperError("device must be a cuda (ROCm) device, got %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.kind, self.num_envs = env_kind, int(num_envs)
        self.obs_dim, self.act_dim, self.words = OBS_DIM[env_kind], ACT_DIM[env_kind], STATE_WORDS[env_kind]
        self.seed, self.env_id_base = int(seed), int(env_id_base)
        self._row_align = 8 if env_kind == ENV_SWING else 16  # float2 / float4 row accesses
        p = (params or default_params()).copy()
        p.flags = (p.flags | F_AUTO_RESET) if auto_reset else (p.flags & ~F_AUTO_RESET)
        self.params = p
        self.auto_reset = bool(auto_reset)
        self.reuse_buffers = bool(reuse_buffers)
        self._h = ctypes.c_void_p()
        # options: a TbOptions, or a dict of make_options() keywords (kernel variants; results never depend on them)
        self.options = options if isinstance(options, TbOptions) else make_options(**(options or {}))
        _check(self.L, self.L.tb_create(ctypes.byref(p), ctypes.byref(self.options), env_kind, self.num_envs, self.device.index, self.seed,
                                        self.env_id_base, ctypes.byref(self._h)), "tb_create")
        self._steps_issued = 0  # agent steps asked of the library so far (capture() measures its K with it)
        n, o = self.num_envs, self.obs_dim
        self._term = torch.zeros((n, o), dtype=torch.float32, device=self.device) if (auto_reset and track_terminal_obs) else None
        self._substeps = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._bufs = None
        # pipelined fast-forward (tb_set_pipeline): terminal rewards of SwingRacket episodes are
        # written later, from a side stream, into the buffers of the step that ended the episode
        self.pipeline = bool(pipeline)
        self._inflight = []
        if self.pipeline:
            if not (auto_reset and env_kind == ENV_SWING):
                raise ValueError("pipeline=True needs SwingRacket-v0 with auto_reset")
            if reuse_buffers:
                raise ValueError("pipeline=True writes late into each step's own buffers: reuse_buffers must be off")
            _check(self.L, self.L.tb_set_pipeline(self._h, 1), "tb_set_pipeline")

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _out(self, T=None):
        t, n, o = self.torch, self.num_envs, self.obs_dim
        lead = (n,) if T is None else (T, n)
        if self.reuse_buffers and T is None:
            if self._bufs is None:
                self._bufs = (t.empty(lead + (o,), dtype=t.float32, device=self.device),
                              t.empty(lead, dtype=t.float32, device=self.device),
                              t.empty(lead, dtype=t.uint8, device=self.device))
            return self._bufs
        return (t.empty(lead + (o,), dtype=t.float32, device=self.device), t.empty(lead, dtype=t.float32, device=self.device),
                t.empty(lead, dtype=t.uint8, device=self.device))

    def _check_tensor(self, x, shape, dtype, name):
        t = self.torch
        if not isinstance(x, t.Tensor):
            raise TypeError("%s must be a torch tensor" % name)
        if x.device != self.device:
            raise ValueError("%s is on %s, the env batch lives on %s" % (name, x.device, self.device))
        if x.dtype != dtype:
            raise TypeError("%s must be %s, got %s" % (name, dtype, x.dtype))
        if tuple(x.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(x.shape)))
        if not x.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        if dtype == t.float32 and x.dim() >= 2 and x.data_ptr() % self._row_align:
            raise ValueError("%s must be %d-byte aligned (the kernels use vector accesses per row)" % (name, self._row_align))
        return x

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.L.tb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ env surface
    def reset(self, mask=None):
        """Start a new episode in every env (or those with mask != 0). Returns obs [N, O]."""
        t = self.torch
        obs = t.empty((self.num_envs, self.obs_dim), dtype=t.float32, device=self.device)
        if mask is not None:
            mask = self._check_tensor(mask.to(t.uint8) if mask.dtype == t.bool else mask, (self.num_envs,), t.uint8, "mask")
            # unmasked rows keep their current observation
            obs.copy_(self.observe())
        _check(self.L, self.L.tb_reset(self._h, None if mask is None else mask.data_ptr(), obs.data_ptr(), self._stream()), "tb_reset")
        return obs

    def step(self, actions, out=None):
        """out: optional (obs, reward, done) tensors to write in place (e.g. slices of a
        RolloutBuffer), shapes [N, O] f32, [N] f32, [N] u8, contiguous, on this device."""
        t = self.torch
        a = self._check_tensor(actions, (self.num_envs, self.act_dim), t.float32, "actions")
        if out is None:
            obs, rew, done = self._out()
        else:
            obs = self._check_tensor(out[0], (self.num_envs, self.obs_dim), t.float32, "out[0]")
            rew = self._check_tensor(out[1], (self.num_envs,), t.float32, "out[1]")
            done = self._check_tensor(out[2], (self.num_envs,), t.uint8, "out[2]")
        _check(self.L, self.L.tb_step(self._h, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(),
                                      None if self._term is None else self._term.data_ptr(),
                                      None if self.pipeline else self._substeps.data_ptr(), self._stream()), "tb_step")
        self._steps_issued += 1
        if self.pipeline and out is None:
            self._inflight.append(rew)  # keep the late-written buffer alive until flush()
            if len(self._inflight) > 4096:
                self.flush()
        return obs, rew, done

    def step_ptrs(self, actions_ptr, obs_ptr, reward_ptr, done_ptr):
        """Unchecked fast path for callers that validated their buffers once (RolloutBuffer.bind):
        raw device addresses of [N, A] f32 actions and [N, O] f32 / [N] f32 / [N] u8 outputs."""
        rc = self.L.tb_step(self._h, actions_ptr, obs_ptr, reward_ptr, done_ptr, None, None,
                            self.torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _check(self.L, rc, "tb_step")
        self._steps_issued += 1

    def step_sequence_ptrs(self, n_steps, actions_ptr, obs_ptr, reward_ptr, done_ptr, strides):
        """n_steps consecutive steps from ONE host call (tb_step_sequence): step t uses the four
        device addresses advanced by t * strides[k] bytes (actions, obs, reward, done). Unchecked
        fast path, like step_ptrs; RolloutBuffer.step_range is the validated caller."""
        rc = self.L.tb_step_sequence(self._h, int(n_steps), actions_ptr, obs_ptr, reward_ptr, done_ptr,
                                     strides[0], strides[1], strides[2], strides[3], self.torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _check(self.L, rc, "tb_step_sequence")
        self._steps_issued += int(n_steps)

    def policy_floats(self, net=NET_DEFAULT):
        """length of the packed policy blob tb_policy_step expects for this env kind and network (NET_DEFAULT, Tennisbot's NET_TUNED,
        SwingRacket's NET_MLP64)"""
        nf = int(self.L.tb_policy_blob_floats(self.kind, check_net(self.kind, net)))
        if nf < 0:
            _check(self.L, nf, "tb_policy_blob_floats")
        return nf

    def policy_step(self, weights, obs_in, seed=0, deterministic=False, out=None, policy_out=None, net=NET_DEFAULT):
        """step() with SB3's MlpPolicy evaluated inside the step kernel (tb_policy_step): each env
        acts on its row of `obs_in`. weights: the packed blob of `ppo.pack_policy`. Returns ((obs, reward, done), (actions, raw_actions, logp, value));
        `out` / `policy_out` are optional tuples of preallocated tensors of those shapes. net: the network the blob holds
        (NET_TUNED: `ppo.build_tuned_actor_critic`, Tennisbot only)."""
        t, n = self.torch, self.num_envs
        nf = self.policy_floats(net)
        w = self._check_tensor(weights, (nf,), t.float32, "weights")
        if w.data_ptr() % 16:
            raise ValueError("weights must be 16-byte aligned")
        oi = self._check_tensor(obs_in, (n, self.obs_dim), t.float32, "obs_in")
        obs, rew, done = self._out() if out is None else out
        self._check_tensor(obs, (n, self.obs_dim), t.float32, "out[0]")
        self._check_tensor(rew, (n,), t.float32, "out[1]")
        self._check_tensor(done, (n,), t.uint8, "out[2]")
        if policy_out is None:
            policy_out = (t.empty((n, self.act_dim), dtype=t.float32, device=self.device), t.empty((n, self.act_dim), dtype=t.float32, device=self.device),
                          t.empty(n, dtype=t.float32, device=self.device), t.empty(n, dtype=t.float32, device=self.device))
        act, raw, logp, value = policy_out
        self._check_tensor(act, (n, self.act_dim), t.float32, "policy_out[0]")
        self._check_tensor(raw, (n, self.act_dim), t.float32, "policy_out[1]")
        self._check_tensor(logp, (n,), t.float32, "policy_out[2]")
        self._check_tensor(value, (n,), t.float32, "policy_out[3]")
        self.policy_step_ptrs(w.data_ptr(), oi.data_ptr(), act.data_ptr(), raw.data_ptr(), logp.data_ptr(), value.data_ptr(),
                              obs.data_ptr(), rew.data_ptr(), done.data_ptr(), seed, deterministic, net)
        if self.pipeline and out is None:
            self._inflight.append(rew)
        return (obs, rew, done), (act, raw, logp, value)

    def policy_step_ptrs(self, weights_ptr, obs_in_ptr, act_ptr, raw_ptr, logp_ptr, value_ptr, obs_ptr, reward_ptr, done_ptr, seed, deterministic=False, net=NET_DEFAULT):
        """unchecked fast path of policy_step (raw device addresses, validated once by the caller)"""
        rc = self.L.tb_policy_step_net(self._h, int(net), weights_ptr, obs_in_ptr, act_ptr, raw_ptr, logp_ptr, value_ptr, obs_ptr, reward_ptr, done_ptr,
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if deterministic else 0, self.torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _check(self.L, rc, "tb_policy_step")
        self._steps_issued += 1

    def mark(self, k):
        """progress mark k (tb_mark_record) at the current stream's position: a counter in pinned host memory goes
        up by one when the stream gets there; together with the library's count of finished fast-forwards it
        tells the host (mark_host_wait) that every step issued so far, late fast-forward writes included, is
        final in the caller's buffers. No stream waits for anything. Inside capture() it is a kernel node that
        every replay fires again."""
        _check(self.L, self.L.tb_mark_record(self._h, int(k), self._stream()), "tb_mark_record")

    def mark_enable(self, on=True):
        """count finished fast-forwards from now on (tb_mark_enable): needed before the steps that marks cover
        are issued or captured; off by default, so plain graphs carry nothing extra"""
        _check(self.L, self.L.tb_mark_enable(self._h, 1 if on else 0), "tb_mark_enable")

    def mark_begin(self):
        """snapshot of the mark counters: call right before launching the work that contains the marks, with
        nothing of this env in flight"""
        _check(self.L, self.L.tb_mark_begin(self._h), "tb_mark_begin")

    def mark_count(self, k):
        """how often mark k has fired so far (a host read)"""
        c = self.L.tb_mark_count(self._h, int(k))
        if c < 0:
            _check(self.L, int(c), "tb_mark_count")
        return int(c)

    def mark_host_wait(self, k, timeout_ms=10000):
        """spin on the host (GIL released) until mark k has fired since mark_begin() and the fast-forwards
        enqueued before it have finished"""
        _check(self.L, self.L.tb_mark_host_wait(self._h, int(k), int(timeout_ms)), "tb_mark_host_wait")

    def policy_rollout_ptrs(self, n_steps, weights_ptr, obs_in_ptr, act_ptr, raw_ptr, logp_ptr, value_ptr, obs_ptr, reward_ptr, done_ptr,
                            strides_bytes, seed, deterministic=False, net=NET_DEFAULT):
        """n_steps of policy_step_ptrs in as few launches as the episodes allow (tb_policy_rollout): the
        towers' weights and the envs' state stay in registers from step to step. strides_bytes: distance
        between consecutive steps of (actions, raw, logp, value, obs, reward, done), 0 = contiguous.
        Unchecked fast path; terminal SwingRacket rewards are complete after flush()."""
        st = (ctypes.c_size_t * 7)(*[int(x) for x in strides_bytes])
        rc = self.L.tb_policy_rollout_net(self._h, int(net), int(n_steps), weights_ptr, obs_in_ptr, act_ptr, raw_ptr, logp_ptr, value_ptr, obs_ptr, reward_ptr, done_ptr,
                                      st, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if deterministic else 0, self.torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _check(self.L, rc, "tb_policy_rollout")
        self._steps_issued += int(n_steps)

    def policy_rollout(self, weights, obs_in, n_steps, seed=0, deterministic=False, net=NET_DEFAULT):
        """T = n_steps agent steps with the MlpPolicy inside the kernel, whole episodes per launch.
        Returns ((obs [T,N,O], reward [T,N], done [T,N]), (actions [T,N,A], raw [T,N,A], logp [T,N], value [T,N]))."""
        t, n, T = self.torch, self.num_envs, int(n_steps)
        w = self._check_tensor(weights, (self.policy_floats(net),), t.float32, "weights")
        oi = self._check_tensor(obs_in, (n, self.obs_dim), t.float32, "obs_in")
        f = dict(dtype=t.float32, device=self.device)
        obs, rew, done = t.empty((T, n, self.obs_dim), **f), t.empty((T, n), **f), t.empty((T, n), dtype=t.uint8, device=self.device)
        act, raw, logp, value = t.empty((T, n, self.act_dim), **f), t.empty((T, n, self.act_dim), **f), t.empty((T, n), **f), t.empty((T, n), **f)
        self.policy_rollout_ptrs(T, w.data_ptr(), oi.data_ptr(), act.data_ptr(), raw.data_ptr(), logp.data_ptr(), value.data_ptr(),
                                 obs.data_ptr(), rew.data_ptr(), done.data_ptr(), (0,) * 7, seed, deterministic, net)
        if self.pipeline:
            self._inflight.append(rew)
        return (obs, rew, done), (act, raw, logp, value)

    def policy_rollout_members_ptrs(self, n_steps, weights_ptr, n_members, weights_stride, envs_per_member, obs_in_ptr, act_ptr, raw_ptr, logp_ptr, value_ptr,
                                    obs_ptr, reward_ptr, done_ptr, strides_bytes, seed, deterministic=False, net=NET_DEFAULT):
        """policy_rollout_ptrs for a population of networks (tb_policy_rollout_members): n_members blobs weights_stride floats
        apart, env i runs with member i // envs_per_member's. Unchecked fast path, validated once by the caller."""
        st = (ctypes.c_size_t * 7)(*[int(x) for x in strides_bytes])
        rc = self.L.tb_policy_rollout_members(self._h, int(net), int(n_steps), weights_ptr, int(n_members), int(weights_stride), int(envs_per_member), obs_in_ptr,
                                              act_ptr, raw_ptr, logp_ptr, value_ptr, obs_ptr, reward_ptr, done_ptr, st, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              1 if deterministic else 0, self.torch.cuda.current_stream(self.device).cuda_stream)
        if rc:
            _check(self.L, rc, "tb_policy_rollout_members")
        self._steps_issued += int(n_steps)

    def policy_rollout_members(self, weights, envs_per_member, obs_in, n_steps, seed=0, deterministic=False, net=NET_DEFAULT):
        """policy_rollout for a population of networks, the same launches (tb_policy_rollout_members). weights: [M, stride] float32
        on this device, row m the packed blob of member m, as policy_evaluate_members takes them (a misaligned, non-contiguous or
        odd-stride input is re-packed first); M * envs_per_member == num_envs, env i uses member i // envs_per_member, and
        envs_per_member must be a multiple of policy_member_granule(). Member m's env columns are what policy_rollout(weights[m])
        gives on a batch of envs_per_member envs at env_id_base + m * envs_per_member. Returns policy_rollout's tuples."""
        t, n, T = self.torch, self.num_envs, int(n_steps)
        weights, M, R = self._members_weights(weights, envs_per_member, self.policy_floats(net))
        oi = self._check_tensor(obs_in, (n, self.obs_dim), t.float32, "obs_in")
        f = dict(dtype=t.float32, device=self.device)
        obs, rew, done = t.empty((T, n, self.obs_dim), **f), t.empty((T, n), **f), t.empty((T, n), dtype=t.uint8, device=self.device)
        act, raw, logp, value = t.empty((T, n, self.act_dim), **f), t.empty((T, n, self.act_dim), **f), t.empty((T, n), **f), t.empty((T, n), **f)
        self.policy_rollout_members_ptrs(T, weights.data_ptr(), M, weights.shape[1], R, oi.data_ptr(), act.data_ptr(), raw.data_ptr(), logp.data_ptr(),
                                         value.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), (0,) * 7, seed, deterministic, net)
        if self.pipeline:
            self._inflight.append(rew)
        return (obs, rew, done), (act, raw, logp, value)

    def es_floats(self):
        """GatedCNN parameters per member for this env kind (766 SwingRacket-v0, 858 Tennisbot-v0)"""
        return int(self.L.tb_es_floats(self.kind))

    def es_evaluate(self, weights, envs_per_member, trace=False, max_steps=None):
        """One episode per env with its member's GatedCNN and a fresh float64 normaliser (tb_es_evaluate; the reference's
        fitness_static). weights: [M, stride] float32 on this device, stride a multiple of 4 and >= es_floats() (pack_population
        in tennisbot_rl_amd/es.py), M * envs_per_member == num_envs; env i uses member i // envs_per_member. Every call resets
        every env first (the episode after the one it was in). Returns (returns float64 [M, R], lengths int32 [M, R]) with
        R = envs_per_member, complete in stream order; with trace=True also a dict of the per-step record
        (net_in / obs [T, N, O], actions / raw [T, N, A], reward [T, N], done [T, N]; rows after an env's last step stay zero),
        T = max_steps or the longest episode (26 / 1001)."""
        t, n = self.torch, self.num_envs
        R = int(envs_per_member)
        if R < 1 or n % R:
            raise ValueError("envs_per_member must divide num_envs (%d)" % n)
        M, P = n // R, self.es_floats()
        if not isinstance(weights, t.Tensor) or weights.dim() != 2 or weights.shape[0] != M:
            raise ValueError("weights must be a [%d, stride] tensor" % M)
        if weights.device != self.device or weights.dtype != t.float32:
            raise ValueError("weights must be float32 on %s" % self.device)
        if weights.shape[1] < P or weights.shape[1] % 4 or not weights.is_contiguous() or weights.data_ptr() % 16:
            w = t.zeros((M, (P + 3) // 4 * 4), dtype=t.float32, device=self.device)
            w[:, :P] = weights[:, :P]
            weights = w
        ret = t.empty(n, dtype=t.float64, device=self.device)
        length = t.empty(n, dtype=t.int32, device=self.device)
        tr, rec = None, None
        if trace:
            T = int(max_steps) if max_steps is not None else (26 if self.kind == ENV_SWING else 1001)
            f = dict(dtype=t.float32, device=self.device)
            rec = dict(net_in=t.zeros((T, n, self.obs_dim), **f), obs=t.zeros((T, n, self.obs_dim), **f), actions=t.zeros((T, n, self.act_dim), **f),
                       raw=t.zeros((T, n, self.act_dim), **f), reward=t.zeros((T, n), **f), done=t.zeros((T, n), dtype=t.uint8, device=self.device))
            tr = TbEsTrace(ctypes.sizeof(TbEsTrace), T, *(rec[k].data_ptr() for k in ("net_in", "obs", "actions", "raw", "reward", "done")))
        _check(self.L, self.L.tb_es_evaluate(self._h, weights.data_ptr(), M, weights.shape[1], R, ret.data_ptr(), length.data_ptr(),
                                             None if tr is None else ctypes.byref(tr), self._stream()), "tb_es_evaluate")
        out = (ret.view(M, R), length.view(M, R))
        return out + (rec,) if trace else out

    def policy_evaluate(self, weights, seed=0, deterministic=False, net=NET_DEFAULT):
        """One whole episode per env with the fused policy inside, in one launch (tb_policy_evaluate). weights: the packed blob of
        `ppo.pack_policy`; sampling, noise keys and clipping are policy_step's, so every env sees the actions a policy_step loop with
        the same seed would have given it. Every call resets every env first (the episode after the one it was in) and leaves every
        env at that episode's freshly reset state. SwingRacket-v0 needs pipeline=True. Returns (returns float64 [N], lengths int32 [N]),
        complete in stream order."""
        t, n = self.torch, self.num_envs
        w = self._check_tensor(weights, (self.policy_floats(net),), t.float32, "weights")
        if w.data_ptr() % 16:
            raise ValueError("weights must be 16-byte aligned")
        ret = t.empty(n, dtype=t.float64, device=self.device)
        length = t.empty(n, dtype=t.int32, device=self.device)
        _check(self.L, self.L.tb_policy_evaluate(self._h, int(net), w.data_ptr(), ret.data_ptr(), length.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                 1 if deterministic else 0, self._stream()), "tb_policy_evaluate")
        return ret, length

    def policy_member_granule(self):
        """envs_per_member of policy_evaluate_members must be a multiple of this (16: the envs of one tower wave)"""
        return int(self.L.tb_policy_member_granule())

    def _members_weights(self, weights, envs_per_member, P, what="a packed policy"):
        """what the members calls ask of [M, stride] rows of P floats each (`what` names them); a misaligned, non-contiguous or odd-stride
        input is re-packed, as es_evaluate does. Returns (weights, M, R)."""
        t, n = self.torch, self.num_envs
        R, G = int(envs_per_member), self.policy_member_granule()
        if R < 1 or R % G:
            raise ValueError("envs_per_member must be a positive multiple of policy_member_granule() (%d), got %d" % (G, R))
        if n % R:
            raise ValueError("envs_per_member must divide num_envs (%d)" % n)
        M, P = n // R, int(P)
        if not isinstance(weights, t.Tensor) or weights.dim() != 2 or weights.shape[0] != M:
            raise ValueError("weights must be a [%d, stride] tensor" % M)
        if weights.device != self.device or weights.dtype != t.float32:
            raise ValueError("weights must be float32 on %s" % self.device)
        if weights.shape[1] < P:
            raise ValueError("weights rows must hold the %d floats of %s, got %d" % (P, what, weights.shape[1]))
        if weights.shape[1] % 4 or not weights.is_contiguous() or weights.data_ptr() % 16:
            w = t.zeros((M, (P + 3) // 4 * 4), dtype=t.float32, device=self.device)
            w[:, :P] = weights[:, :P]
            weights = w
        return weights, M, R

    def policy_evaluate_members(self, weights, envs_per_member, seed=0, deterministic=False, net=NET_DEFAULT):
        """policy_evaluate for a population of networks in one launch (tb_policy_evaluate_members). weights: [M, stride] float32 on
        this device, row m the packed blob of member m (`ppo.pack_policy`; `policy_es.pack_policy_members` for perturbations of one
        policy), stride a multiple of 4 and >= policy_floats(net); M * envs_per_member == num_envs and env i uses member
        i // envs_per_member; envs_per_member must be a multiple of policy_member_granule(). A misaligned, non-contiguous or
        short-stride input is re-packed first, as es_evaluate does. Sampling, noise keys, the reset in front and the state
        afterwards are policy_evaluate's: row m is what policy_evaluate(weights[m]) gives on a batch of envs_per_member envs at
        env_id_base + m * envs_per_member. Returns (returns float64 [M, R], lengths int32 [M, R]), complete in stream order."""
        t, n = self.torch, self.num_envs
        weights, M, R = self._members_weights(weights, envs_per_member, self.policy_floats(net))
        ret = t.empty(n, dtype=t.float64, device=self.device)
        length = t.empty(n, dtype=t.int32, device=self.device)
        _check(self.L, self.L.tb_policy_evaluate_members(self._h, int(net), weights.data_ptr(), M, weights.shape[1], R, ret.data_ptr(), length.data_ptr(),
                                                         int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if deterministic else 0, self._stream()), "tb_policy_evaluate_members")
        return ret.view(M, R), length.view(M, R)

    def sac_actor_floats(self):
        """Floats of the flat SAC / TQC actor vector for this env kind (70668 SwingRacket-v0, 70148 Tennisbot-v0)"""
        return int(self.L.tb_sac_param_floats(self.kind, 0))

    def sac_evaluate(self, actor_flat, seed=0, deterministic=False, trace=False, max_steps=None):
        """One whole episode per env with the SAC / TQC actor inside, in one launch (tb_sac_evaluate). actor_flat: the flat
        TB_SAC_ACTOR vector (named_parameters() order, as the learner trains it), float32 on this device. Per step
        a = tanh(mu + exp(clamp(log_std, -20, 2)) eps) with policy_step's noise keys (seed, env id, episode, step);
        deterministic=True acts on tanh(mu). Every call resets every env first (the episode after the one it was in) and leaves
        every env at that episode's freshly reset state. SwingRacket-v0 needs pipeline=True. Returns (returns float64 [N],
        lengths int32 [N]), complete in stream order; with trace=True also a dict of the per-step record (obs [T, N, O], eps /
        actions [T, N, A], reward [T, N], done [T, N]; rows after an env's last step stay zero), T = max_steps or the longest
        episode (26 / 1001). The trace never changes a result."""
        t, n = self.torch, self.num_envs
        w = self._check_tensor(actor_flat, (self.sac_actor_floats(),), t.float32, "actor_flat")
        ret = t.empty(n, dtype=t.float64, device=self.device)
        length = t.empty(n, dtype=t.int32, device=self.device)
        tr, rec = self._sac_eval_trace(trace, max_steps)
        _check(self.L, self.L.tb_sac_evaluate(self._h, w.data_ptr(), ret.data_ptr(), length.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              1 if deterministic else 0, None if tr is None else ctypes.byref(tr), self._stream()), "tb_sac_evaluate")
        return (ret, length, rec) if trace else (ret, length)

    def _sac_eval_trace(self, trace, max_steps):
        """(TbSacEvalTrace or None, the dict of zeroed [T, N, ...] arrays it points into or None) for sac_evaluate / sac_evaluate_members"""
        if not trace:
            return None, None
        t, n = self.torch, self.num_envs
        T = int(max_steps) if max_steps is not None else (26 if self.kind == ENV_SWING else 1001)
        f = dict(dtype=t.float32, device=self.device)
        rec = dict(obs=t.zeros((T, n, self.obs_dim), **f), eps=t.zeros((T, n, self.act_dim), **f), actions=t.zeros((T, n, self.act_dim), **f),
                   reward=t.zeros((T, n), **f), done=t.zeros((T, n), dtype=t.uint8, device=self.device))
        return TbSacEvalTrace(ctypes.sizeof(TbSacEvalTrace), T, *(rec[k].data_ptr() for k in ("obs", "eps", "actions", "reward", "done"))), rec

    def sac_evaluate_members(self, actors, envs_per_member, seed=0, deterministic=False, trace=False, max_steps=None):
        """sac_evaluate for a population of actors in one launch (tb_sac_evaluate_members). actors: [M, stride] float32 on this
        device, row m the flat TB_SAC_ACTOR vector of member m, stride a multiple of 4 and >= sac_actor_floats();
        M * envs_per_member == num_envs and env i uses member i // envs_per_member; envs_per_member must be a multiple of
        policy_member_granule(). A misaligned, non-contiguous or odd-stride input is re-packed first, as es_evaluate does. Sampling,
        noise keys, the reset in front and the state afterwards are sac_evaluate's: row m is what sac_evaluate(actors[m]) gives on a
        batch of envs_per_member envs at env_id_base + m * envs_per_member. Returns (returns float64 [M, R], lengths int32 [M, R]),
        complete in stream order; with trace=True also sac_evaluate's dict, its rows [T, M * R, ...] in env order."""
        t, n = self.torch, self.num_envs
        actors, M, R = self._members_weights(actors, envs_per_member, self.sac_actor_floats(), "a flat SAC / TQC actor")
        ret = t.empty(n, dtype=t.float64, device=self.device)
        length = t.empty(n, dtype=t.int32, device=self.device)
        tr, rec = self._sac_eval_trace(trace, max_steps)
        _check(self.L, self.L.tb_sac_evaluate_members(self._h, actors.data_ptr(), M, actors.shape[1], R, ret.data_ptr(), length.data_ptr(),
                                                      int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if deterministic else 0, None if tr is None else ctypes.byref(tr),
                                                      self._stream()), "tb_sac_evaluate_members")
        return (ret.view(M, R), length.view(M, R), rec) if trace else (ret.view(M, R), length.view(M, R))

    def sac_collect(self, actor_flat, n_steps, out_views, seed=0, uniform=False, eps=None):
        """n_steps agent steps of every env from where it stands, in one launch with the SAC / TQC actor inside, every transition
        written as a replay ring stores it (tb_sac_collect). actor_flat: the flat TB_SAC_ACTOR vector, or None with uniform=True
        (actions uniform in [-1, 1), from the Philox words of the same keys). out_views = (obs, next_obs, action, reward, done):
        contiguous float32 tensors [S, N, O], [S, N, O], [S, N, A], [S, N], [S, N] on this device (S * N leading rows also do:
        views of a ring), done as 0.0 / 1.0; eps: optional [S, N, A] for the noise drawn. Envs that finish restart inside the
        launch and the state is written back, as n_steps calls of step() would leave it. SwingRacket-v0 needs pipeline=True, envs
        in lockstep and phase() + n_steps <= 26; every output is complete in stream order on return (no flush() needed)."""
        t, n, S = self.torch, self.num_envs, int(n_steps)
        if S < 1:
            raise ValueError("n_steps must be >= 1")
        if len(out_views) != 5:
            raise ValueError("out_views must be (obs, next_obs, action, reward, done)")
        dims = (self.obs_dim, self.obs_dim, self.act_dim, None, None)
        names = ("obs", "next_obs", "action", "reward", "done")
        views = list(zip(names, out_views, dims)) + ([("eps", eps, self.act_dim)] if eps is not None else [])
        for name, x, k in views:
            if not isinstance(x, t.Tensor) or x.device != self.device or x.dtype != t.float32 or not x.is_contiguous():
                raise ValueError("%s must be a contiguous float32 tensor on %s" % (name, self.device))
            if x.numel() != S * n * (k or 1) or (k is not None and x.shape[-1] != k):
                raise ValueError("%s must hold %d x %d rows%s, got %s" % (name, S, n, "" if k is None else " of %d" % k, tuple(x.shape)))
        w = None
        if not uniform:
            w = self._check_tensor(actor_flat, (self.sac_actor_floats(),), t.float32, "actor_flat")
        out = TbSacCollectOut(ctypes.sizeof(TbSacCollectOut), *(x.data_ptr() for x in out_views), None if eps is None else eps.data_ptr())
        _check(self.L, self.L.tb_sac_collect(self._h, None if w is None else w.data_ptr(), S, SAC_COLLECT_UNIFORM if uniform else SAC_COLLECT_ACTOR,
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(out), self._stream()), "tb_sac_collect")
        self._steps_issued += S

    def capture(self, fn):
        """Capture `fn()` -- a fixed sequence of step()/step_ptrs()/RolloutBuffer.step_into calls on
        fixed buffers -- into a HIP graph and return it as a StepGraph; `graph.replay()` then runs the
        whole sequence with one launch (no per-step host work). In pipelined mode the side-stream
        fast-forwards are captured as forked branches and joined by the final flush(). Nothing runs
        during the capture: the env (and the library's episode phase) are where they were, and the
        first replay() is the first time the steps happen."""
        t = self.torch
        if self.pipeline:
            self.flush()  # (also runs the pool of deferred stragglers, if any: nothing of this env may be pending across the capture boundary)
        t.cuda.current_stream(self.device).synchronize()
        _check(self.L, self.L.tb_pipeline_sync(self._h, 1), "tb_pipeline_sync")
        phase = self.L.tb_phase(self._h) if self.pipeline else -1
        gen = self.L.tb_params_generation(self._h)
        issued = self._steps_issued
        g = t.cuda.CUDAGraph()
        try:
            # thread_local: other threads (e.g. the RCCL watchdog of torch.distributed) may keep
            # issuing HIP calls while this thread captures
            with t.cuda.graph(g, capture_error_mode="thread_local"):
                fn()
                self.flush()
        except BaseException:
            # nothing captured ever ran; put the handle's streams and phase hint back (the env is intact)
            try:
                t.cuda.synchronize(self.device)
            except Exception:  # the capture error may surface once more through torch
                pass
            self.L.tb_pipeline_recover(self._h)
            self._steps_issued = issued
            raise
        _check(self.L, self.L.tb_pipeline_sync(self._h, 0), "tb_pipeline_sync")  # also puts the phase back: nothing ran
        n_steps, self._steps_issued = self._steps_issued - issued, issued
        return StepGraph(self, g, n_steps, phase, gen)

    def flush(self):
        """Pipelined mode: make the current stream wait until every outstanding fast-forward has
        written its step's reward / terminal observation / substep count."""
        _check(self.L, self.L.tb_flush(self._h, self._stream()), "tb_flush")
        self._inflight = []

    def rollout(self, actions):
        """T steps in one launch: actions [T, N, A] -> obs [T, N, O], reward [T, N], done [T, N]."""
        t = self.torch
        if actions.dim() != 3:
            raise ValueError("actions must be [T, N, A]")
        T = int(actions.shape[0])
        a = self._check_tensor(actions, (T, self.num_envs, self.act_dim), t.float32, "actions")
        obs, rew, done = self._out(T)
        _check(self.L, self.L.tb_rollout(self._h, T, a.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(),
                                         None if self.pipeline else self._substeps.data_ptr(), self._stream()), "tb_rollout")
        self._steps_issued += T
        if self.pipeline:
            self._inflight.append(rew)  # terminal rewards are written late, from the side streams: flush() before reading
        return obs, rew, done

    def terminal_obs(self):
        """[N, O]: for envs whose episode ended in the latest step, its final observation."""
        if self._term is None:
            raise StepperError("terminal observations are only tracked with auto_reset=True")
        if self.pipeline:
            self.flush()
        return self._term

    def last_substeps(self):
        """int32 [N]: physics substeps executed by the latest step()/rollout() call."""
        if self.pipeline:
            raise StepperError("per-step substep counts are not tracked in pipelined mode (use counters()['substeps'])")
        return self._substeps

    def observe(self):
        """Current observation rebuilt from the state (no stepping)."""
        t = self.torch
        w, _ = self.get_state_words()
        f = w.view(t.float32)
        if self.kind == ENV_SWING:
            rows = [0, 1, 13, 14, 22, 23]
        else:
            rows = [0, 1, 2, 7, 8, 9, 13, 14, 15, 16, 17, 18]
        return f[rows].t().contiguous()

    def render(self, indices=None, camera=None, width=96, height=64, layers=False):
        """rgb_array frames of the envs as they stand (tb_render: one ray per pixel against ground, net, goal, ball and racket, one
        launch for every image). Returns uint8 [K, H, W, 3] on the device, K = len(indices) or num_envs; with layers=True also ids
        uint8 [K, H, W] (RENDER_IDS) and depth float32 [K, H, W] (+inf: sky). camera: Camera(...) / default_camera(kind) /
        racket_view(...). It works from get_state_words() -- on a pipelined SwingRacket handle that joins the outstanding
        fast-forwards, as every state read does -- and writes nothing of the env: state, counters and the next step are untouched."""
        w, _ = self.get_state_words()
        return render_words(self.kind, self.params, w, indices=indices, camera=camera, width=width, height=height, layers=layers)

    def trace_step(self, actions, stride=8, words=None, done=None, max_frames=None):
        """One SwingRacket-v0 agent step with the states it passes through (tb_swing_trace): the 26th step's fast-forward -- the ball's
        whole flight, up to 775 substeps -- sampled every `stride` substeps. words / done: the states to step, int32 [W, K] and uint8
        [K] in get_state_words' layout (done=None: all running); words=None traces this env's own current state, read as
        get_state_words reads it (a pipelined handle joins its outstanding fast-forwards first). actions: float32 [K, 6]. Nothing of
        this env changes: state, counters, phase and the next step are what they were. Returns a dict of device tensors, complete in
        stream order: frames int32 [F, W, K] (F = max_frames, default 2 + 775 // stride: any flight and a row to spare; frames[k]
        feeds render_words as it is), n_frames int32 [K] (samples per env, trace_frame_substeps' rule; rows behind them repeat the
        final state), and reward float32 [K], substeps int32 [K], done uint8 [K], obs float32 [K, 6] -- what set_state_words(words,
        done) and step(actions) give on an env without auto-reset, bit for bit."""
        if self.kind != ENV_SWING:
            raise ValueError("trace_step is SwingRacket-v0's: every Tennisbot-v0 agent step is one substep and is visible as it is")
        t = self.torch
        stride = int(stride)
        F = 2 + (TRACE_MAX_SUBSTEPS - 1) // max(stride, 1) if max_frames is None else int(max_frames)
        if words is None:
            if done is not None:
                raise ValueError("done belongs to words: give both, or neither to trace the env's own state")
            w, d = self.get_state_words()
        else:
            w = words if isinstance(words, t.Tensor) else t.from_numpy(np.ascontiguousarray(words).view(np.int32))
            w = w.to(self.device)
            if w.dim() != 2 or w.shape[0] != self.words or w.element_size() != 4 or not w.is_contiguous():
                raise ValueError("words must be a contiguous [%d, K] tensor of 32-bit words" % self.words)
            if done is None:
                d = t.zeros(int(w.shape[1]), dtype=t.uint8, device=self.device)
            else:
                d = done if isinstance(done, t.Tensor) else t.from_numpy(np.ascontiguousarray(done, np.uint8))
                d = self._check_tensor(d.to(self.device).contiguous(), (int(w.shape[1]),), t.uint8, "done")
        K = int(w.shape[1])
        a = self._check_tensor(actions, (K, self.act_dim), t.float32, "actions")
        out = dict(frames=t.empty((max(F, 0), self.words, K), dtype=t.int32, device=self.device),   # (a size < 1 is the library's to refuse)
                   n_frames=t.empty(K, dtype=t.int32, device=self.device), reward=t.empty(K, dtype=t.float32, device=self.device),
                   substeps=t.empty(K, dtype=t.int32, device=self.device), done=t.empty(K, dtype=t.uint8, device=self.device),
                   obs=t.empty((K, self.obs_dim), dtype=t.float32, device=self.device))
        _check(self.L, self.L.tb_swing_trace(self._h, w.data_ptr(), d.data_ptr(), K, a.data_ptr(), stride, F, out["frames"].data_ptr(),
                                             out["n_frames"].data_ptr(), out["reward"].data_ptr(), out["substeps"].data_ptr(),
                                             out["done"].data_ptr(), out["obs"].data_ptr(), self._stream()), "tb_swing_trace")
        return out

    def set_params(self, params):
        p = params.copy()
        p.flags = (p.flags | F_AUTO_RESET) if self.auto_reset else (p.flags & ~F_AUTO_RESET)
        _check(self.L, self.L.tb_set_params(self._h, ctypes.byref(p), self._stream()), "tb_set_params")
        self.params = p

    def set_racket_scale(self, scale):
        """tennisbot_env.py:213-215: takes effect at the next reset of each env (the reference
        rebuilds the racket with globalScaling=scale in reset(), :230-234); every env keeps the
        scale of its current episode in its own state word. One stream-ordered store into the
        device-resident parameter block (tb_set_racket_scale): graphs captured earlier see it."""
        _check(self.L, self.L.tb_set_racket_scale(self._h, float(scale), self._stream()), "tb_set_racket_scale")
        self.params.racket_scale = float(scale)

    def phase(self):
        """agent steps since the last common reset modulo 26, or -1 when the envs are not in lockstep"""
        return int(self.L.tb_phase(self._h))

    PIPELINE_FORMS = ("none", "slots", "slots+pool", "pool")

    def pipeline_form(self):
        """tb_pipeline_form as a word: "none" (fast-forward inside the 26th step), "slots" (one fast-forward kernel per episode end on a
        side stream), "slots+pool" (its stragglers deferred to the join), "pool" (every episode end parked, ONE fast-forward at the join)"""
        return self.PIPELINE_FORMS[int(self.L.tb_pipeline_form(self._h))]

    def step_waves(self):
        """tb_step_waves: waves per 64 envs of the pipelined SwingRacket one-step kernel, 2 (racket and ball on waves of their own) or 1;
        0 without that kernel"""
        return int(self.L.tb_step_waves(self._h))

    def step_form(self):
        """tb_step_form: which form of that kernel the next step() launches -- 0 one-wave, 1 two-wave with the early gate, 2 two-wave
        short (lockstep episodes, not their last step); -1 without that kernel"""
        return int(self.L.tb_step_form(self._h))

    # ------------------------------------------------------------------ state save / restore
    def get_state_words(self):
        t = self.torch
        w = t.empty((self.words, self.num_envs), dtype=t.int32, device=self.device)
        d = t.empty(self.num_envs, dtype=t.uint8, device=self.device)
        _check(self.L, self.L.tb_get_state(self._h, w.data_ptr(), d.data_ptr(), 1, self._stream()), "tb_get_state")
        return w, d

    def set_state_words(self, words, done=None):
        t = self.torch
        w = words if isinstance(words, t.Tensor) else t.from_numpy(np.ascontiguousarray(words).view(np.int32))
        w = self._check_tensor(w.to(self.device).contiguous(), (self.words, self.num_envs), t.int32, "words")
        dptr = None
        if done is not None:
            d = done if isinstance(done, t.Tensor) else t.from_numpy(np.ascontiguousarray(done, np.uint8))
            d = self._check_tensor(d.to(self.device).contiguous(), (self.num_envs,), t.uint8, "done")
            dptr = d.data_ptr()
        _check(self.L, self.L.tb_set_state(self._h, w.data_ptr(), dptr, 1, self._stream()), "tb_set_state")
        self.torch.cuda.current_stream(self.device).synchronize()  # the source tensors may be temporaries

    def get_state(self):
        """dict of named numpy arrays (host copy): the env checkpoint the reference never had."""
        w, d = self.get_state_words()
        w = w.cpu().numpy().view(np.uint32)
        names = STATE_ROWS[self.kind]
        out, i = {}, 0
        fl = w.view(np.float32)
        while i < len(names):
            j = i
            while j < len(names) and names[j] == names[i]:
                j += 1
            out[names[i]] = np.ascontiguousarray(fl[i:j].T)
            i = j
        out["step_count"] = w[self.words - 2].view(np.int32).copy()
        out["episode"] = w[self.words - 1].copy()
        if "init_dist" in out:
            out["init_dist"] = out["init_dist"][:, 0]
        out["done"] = d.cpu().numpy()
        return out

    def save_state(self, path):
        """on-disk checkpoint of the env batch (npz): raw SoA words + done bytes + identity"""
        w, d = self.get_state_words()
        np.savez_compressed(path, words=w.cpu().numpy(), done=d.cpu().numpy(), env_kind=self.kind, num_envs=self.num_envs,
                            seed=self.seed, env_id_base=self.env_id_base, rows=np.array(STATE_ROWS[self.kind]))

    def load_state(self, path):
        z = np.load(path, allow_pickle=False)
        if int(z["env_kind"]) != self.kind or int(z["num_envs"]) != self.num_envs:
            raise ValueError("checkpoint is for env kind %d x %d envs" % (int(z["env_kind"]), int(z["num_envs"])))
        self.set_state_words(z["words"], z["done"])

    def counters(self):
        c = (ctypes.c_uint64 * N_COUNTERS)()
        _check(self.L, self.L.tb_counters(self._h, c, self._stream()), "tb_counters")
        return dict(zip(COUNTER_NAMES, [int(x) for x in c]))

    def sealed_substeps(self):
        """how many of counters()['substeps'] the pool's sealed-fate exit booked without running them (TbOptions.ff_seal)"""
        c = ctypes.c_uint64(0)
        _check(self.L, self.L.tb_sealed_substeps(self._h, ctypes.byref(c), self._stream()), "tb_sealed_substeps")
        return int(c.value)

    def counters_reset(self):
        _check(self.L, self.L.tb_counters_reset(self._h, self._stream()), "tb_counters_reset")
