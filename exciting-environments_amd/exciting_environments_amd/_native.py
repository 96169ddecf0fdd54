"""ctypes binding of libexcenv_hip.so (C ABI: include/excenv.h).

This is the only compute backend of the package. There is no CPU or PyTorch fallback: if the
shared library is missing, or no HIP device is present when a kernel entry point is called, the
call raises.

One convention for every entry point: `PROTOTYPES` gives each function of the header its restype and argtypes, so callers pass
plain Python ints / floats / None, `byref()` results and pointer arrays (a bare int for a pointer argument is converted as a
64-bit address, never truncated). The constants and structures below mirror the header; tests/test_native_binding.py compares
them with it (values, sizes, field offsets, argument counts).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import torch

MAX_STATE, MAX_ACTION, MAX_STATIC, MAX_CONTROL = 8, 2, 9, 8
LAYOUT_ENV_MAJOR, LAYOUT_LANE_MAJOR, LAYOUT_TILED = 0, 1, 2
TILE = 1024  # EXCENV_TILE
SEM_STEP, SEM_AHEAD = 0, 1
SEM_AHEAD_ACCUMULATED_T = 2  # opt-in: diffrax's accumulated-time clock as the CPU oracle restates it (include/excenv.h)
# CoreEnvironment.sim_ahead_semantics -> excenv_semantics_t
SEMANTICS = {"step": SEM_STEP, "ahead": SEM_AHEAD, "ahead_accumulated_t": SEM_AHEAD_ACCUMULATED_T}
F32, F64 = 0, 1
JAC_STATE, JAC_OBS = 0, 1  # excenv_jac_rows_t: the rows of excenv_step_jacobian
JAC_ROWS = {"state": JAC_STATE, "obs": JAC_OBS}
OPT_NO_FUSED_ACTIONS = 1  # EXCENV_OPT_NO_FUSED_ACTIONS
OPT_KEEP_CONSTANT_COLUMNS = 2  # EXCENV_OPT_KEEP_CONSTANT_COLUMNS
ABI_VERSION = 7
POLICY_MAX_LAYERS, POLICY_MAX_WIDTH = 4, 64  # excenv_policy_t: linear layers of the MLP, units of a hidden layer
POLICY_MAX_INPUT = 16  # excenv_policy_param_grad: the widest observation row, 8 + MAX_CONTROL
PARAM_GRAD_CHAIN = 4096  # samples one working-dtype accumulator of policy_param_grad_kernel sums before it goes to fp64
PARAM_GRAD_AUTO_GROUPS = 512  # its workgroups with max_groups == 0, at most
PPO_STATS = 5  # excenv_ppo_loss: n, S_surr, S_vsq, S_kl, S_clip in front of S_gls[A]
PPO_TILE = 1024  # samples of one tile of the PPO kernels: consecutive environments of one row
PPO_AUTO_GROUPS = 2048  # workgroups of excenv_ppo_loss with max_groups == 0, at most
MOMENTS_MAX_COLUMNS = 16  # excenv_row_moments: the widest row, C
EPISODE_STATS = 6  # excenv_episode_stats: cnt, SR, SRR, SL, mn, mx
LQR_SHAPES = ((1, 1), (2, 1), (4, 1), (7, 2))  # excenv_lqr_backward: the (n_state, n_action) riccati_kernel is instantiated for
ACT_RELU, ACT_TANH = 0, 1
ACTIVATIONS = {"relu": ACT_RELU, "tanh": ACT_TANH}
END_TERMINATED, END_TRUNCATED = 1, 2  # excenv_episode_t.end_mask
END_ON = {"terminated": END_TERMINATED, "truncated": END_TRUNCATED}

_LIB_PATH = os.environ.get(  # EXCENV_HIP_LIB: A/B-test another build of the same library (tuning experiments)
    "EXCENV_HIP_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libexcenv_hip.so"))


class Param(ctypes.Structure):
    _fields_ = [("value", ctypes.c_double), ("per_env", ctypes.c_void_p)]


class PmsmLut(ctypes.Structure):
    _fields_ = [("n_d", ctypes.c_int32), ("n_q", ctypes.c_int32), ("grid_d", ctypes.c_void_p),
                ("grid_q", ctypes.c_void_p), ("tables", ctypes.c_void_p)]


class Props(ctypes.Structure):
    _fields_ = [
        ("static_params", Param * MAX_STATIC),
        ("state_min", Param * MAX_STATE),
        ("state_max", Param * MAX_STATE),
        ("action_min", Param * MAX_ACTION),
        ("action_max", Param * MAX_ACTION),
        ("pmsm_lut", ctypes.POINTER(PmsmLut)),
    ]


class LaunchOpts(ctypes.Structure):
    """excenv_launch_opts_t: per-call launch shaping (None / NULL = defaults)."""

    _fields_ = [("envs_per_lane", ctypes.c_int32), ("env_major_mode", ctypes.c_int32), ("lds_pad_bytes", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


class TrajGym(ctypes.Structure):
    """excenv_traj_gym_t: optional reward / terminated / truncated trajectories of excenv_sim_ahead."""

    _fields_ = [("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p), ("truncated", ctypes.c_void_p)]


class Control(ctypes.Structure):
    _fields_ = [
        ("n_control", ctypes.c_int32),
        ("control_idx", ctypes.c_int32 * MAX_CONTROL),
        ("reference", ctypes.c_void_p * MAX_CONTROL),
        ("obs_reference", ctypes.c_void_p * MAX_CONTROL),  # gym_step only: NULL = the observation shows `reference`
    ]


class Feedback(ctypes.Structure):
    """excenv_feedback_t: the affine feedback policy of excenv_sim_feedback (gains, feedforward, integrator state, clamp)."""

    _fields_ = [("gain", ctypes.c_void_p), ("integral_gain", ctypes.c_void_p), ("gain_batch", ctypes.c_int64),
                ("feedforward", ctypes.c_void_p), ("z_in", ctypes.c_void_p), ("z_out", ctypes.c_void_p),
                ("clip_lo", ctypes.c_double), ("clip_hi", ctypes.c_double)]


class FeedbackVjp(ctypes.Structure):
    """excenv_feedback_vjp_t: the stored forward of one excenv_sim_feedback call, the cotangents of its outputs and where the
    gradients go (excenv_sim_feedback_vjp)."""

    _fields_ = [("gain", ctypes.c_void_p), ("integral_gain", ctypes.c_void_p), ("gain_batch", ctypes.c_int64),
                ("clip_lo", ctypes.c_double), ("clip_hi", ctypes.c_double), ("obs_traj", ctypes.c_void_p),
                ("state_traj", ctypes.c_void_p), ("actions", ctypes.c_void_p), ("z_in", ctypes.c_void_p),
                ("grad_obs", ctypes.c_void_p), ("grad_states", ctypes.c_void_p), ("grad_last_state", ctypes.c_void_p),
                ("grad_actions", ctypes.c_void_p), ("grad_z", ctypes.c_void_p), ("grad_state0", ctypes.c_void_p),
                ("grad_ff", ctypes.c_void_p), ("grad_zi", ctypes.c_void_p), ("grad_z0", ctypes.c_void_p),
                ("grad_gain", ctypes.c_void_p), ("grad_integral_gain", ctypes.c_void_p)]


class Policy(ctypes.Structure):
    """excenv_policy_t: the MLP policy of excenv_sim_policy (one shared parameter array, widths, activation, noise rows, clamp)."""

    _fields_ = [("params", ctypes.c_void_p), ("n_layers", ctypes.c_int32), ("activation", ctypes.c_int32),
                ("widths", ctypes.c_int32 * (POLICY_MAX_LAYERS + 1)), ("noise", ctypes.c_void_p), ("clip_lo", ctypes.c_double),
                ("clip_hi", ctypes.c_double)]


class PolicyVjp(ctypes.Structure):
    """excenv_policy_vjp_t: the policy record and the stored forward of one excenv_sim_policy call, the cotangents of its outputs
    and where the gradients go (excenv_sim_policy_vjp)."""

    _fields_ = [("policy", Policy), ("obs_traj", ctypes.c_void_p), ("state_traj", ctypes.c_void_p), ("actions", ctypes.c_void_p),
                ("reset", ctypes.c_void_p), ("grad_obs", ctypes.c_void_p), ("grad_states", ctypes.c_void_p),
                ("grad_last_state", ctypes.c_void_p), ("grad_actions", ctypes.c_void_p), ("grad_state0", ctypes.c_void_p),
                ("grad_raw", ctypes.c_void_p)]


class PolicyParamGrad(ctypes.Structure):
    """excenv_policy_param_grad_t: the network, the saved observation rows, the cotangent rows excenv_sim_policy_vjp wrote, where the
    parameter gradient goes and the workspace of the two launches (excenv_policy_param_grad)."""

    _fields_ = [("policy", Policy), ("obs_traj", ctypes.c_void_p), ("grad_raw", ctypes.c_void_p), ("grad_params", ctypes.c_void_p),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64), ("max_groups", ctypes.c_int32)]


class PolicyEval(ctypes.Structure):
    """excenv_policy_eval_t: the network, the stored observation rows and where its raw outputs go (excenv_policy_eval)."""

    _fields_ = [("policy", Policy), ("obs_traj", ctypes.c_void_p), ("out", ctypes.c_void_p)]


class Gae(ctypes.Structure):
    """excenv_gae_t: lane-major reward / value rows, the optional flag bytes, the two discounts and the outputs (excenv_gae)."""

    _fields_ = [("reward", ctypes.c_void_p), ("value", ctypes.c_void_p), ("terminated", ctypes.c_void_p), ("reset", ctypes.c_void_p),
                ("gamma", ctypes.c_double), ("lambda", ctypes.c_double), ("advantage", ctypes.c_void_p), ("returns", ctypes.c_void_p)]


class GaussianLogp(ctypes.Structure):
    """excenv_gaussian_logp_t: lane-major means and samples, the reciprocal deviations and the constant, and where the
    log-probabilities go (excenv_gaussian_logp)."""

    _fields_ = [("mean", ctypes.c_void_p), ("sample", ctypes.c_void_p), ("inv_std", ctypes.c_void_p), ("logp_const", ctypes.c_void_p),
                ("n_actions", ctypes.c_int32), ("logp", ctypes.c_void_p)]


class PpoLoss(ctypes.Structure):
    """excenv_ppo_loss_t: the lane-major rows of a PPO update, the clip range, the sums and workspace of excenv_ppo_loss and the
    scales and outputs of excenv_ppo_loss_grad."""

    _fields_ = [("mean", ctypes.c_void_p), ("sample", ctypes.c_void_p), ("inv_std", ctypes.c_void_p), ("logp_const", ctypes.c_void_p),
                ("logp_old", ctypes.c_void_p), ("advantage", ctypes.c_void_p), ("value", ctypes.c_void_p), ("returns", ctypes.c_void_p),
                ("reset", ctypes.c_void_p), ("adv_norm", ctypes.c_void_p), ("n_actions", ctypes.c_int32), ("max_groups", ctypes.c_int32),
                ("clip_eps", ctypes.c_double), ("stats", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
                ("workspace_bytes", ctypes.c_int64), ("grad_scale", ctypes.c_void_p), ("grad_mean", ctypes.c_void_p),
                ("grad_value", ctypes.c_void_p)]


class RowMoments(ctypes.Structure):
    """excenv_row_moments_t: lane-major rows, the optional mask bytes and shifts, the sums and the workspace (excenv_row_moments)."""

    _fields_ = [("x", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("n_columns", ctypes.c_int32),
                ("max_groups", ctypes.c_int32), ("stats", ctypes.c_void_p), ("workspace", ctypes.c_void_p),
                ("workspace_bytes", ctypes.c_int64)]


class EpisodeStats(ctypes.Structure):
    """excenv_episode_stats_t: lane-major rewards and reset bytes, the two carries in and out, the per-row returns, the six statistics
    and the workspace (excenv_episode_stats)."""

    _fields_ = [("reward", ctypes.c_void_p), ("reset", ctypes.c_void_p), ("return_in", ctypes.c_void_p), ("steps_in", ctypes.c_void_p),
                ("completed", ctypes.c_void_p), ("return_out", ctypes.c_void_p), ("steps_out", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64)]


class Lqr(ctypes.Structure):
    """excenv_lqr_t: the stored Jacobians, the cost matrices and linear terms, and the outputs of the Riccati recursion
    (excenv_lqr_backward)."""

    _fields_ = [("n_state", ctypes.c_int32), ("n_action", ctypes.c_int32), ("jac", ctypes.c_void_p), ("jac_row_stride", ctypes.c_int64),
                ("Q", ctypes.c_void_p), ("Qf", ctypes.c_void_p), ("R", ctypes.c_void_p), ("q", ctypes.c_void_p), ("r", ctypes.c_void_p),
                ("reg", ctypes.c_double), ("store_all", ctypes.c_int32), ("gain", ctypes.c_void_p), ("ff", ctypes.c_void_p),
                ("P0", ctypes.c_void_p), ("p0", ctypes.c_void_p), ("dV", ctypes.c_void_p), ("n_bad", ctypes.c_void_p)]


class Episode(ctypes.Structure):
    """excenv_episode_t: the reset rows, the end conditions and the gym / reset outputs of excenv_sim_policy_episodes."""

    _fields_ = [("reset_states", ctypes.c_void_p), ("n_reset_rows", ctypes.c_int32), ("end_mask", ctypes.c_int32),
                ("max_episode_steps", ctypes.c_int32), ("episode_steps_in", ctypes.c_void_p), ("reward", ctypes.c_void_p),
                ("terminated", ctypes.c_void_p), ("truncated", ctypes.c_void_p), ("reset", ctypes.c_void_p),
                ("n_resets", ctypes.c_void_p), ("episode_steps_out", ctypes.c_void_p)]


# the C types of the header's structures (tests/test_native_binding.py compares sizes and field offsets with the host compiler's)
STRUCTS = {Param: "excenv_param_t", PmsmLut: "excenv_pmsm_lut_t", Props: "excenv_props_t", LaunchOpts: "excenv_launch_opts_t",
           TrajGym: "excenv_traj_gym_t", Control: "excenv_control_t", Feedback: "excenv_feedback_t",
           FeedbackVjp: "excenv_feedback_vjp_t", Policy: "excenv_policy_t", Episode: "excenv_episode_t",
           PolicyVjp: "excenv_policy_vjp_t", PolicyParamGrad: "excenv_policy_param_grad_t", PolicyEval: "excenv_policy_eval_t",
           Gae: "excenv_gae_t", GaussianLogp: "excenv_gaussian_logp_t", PpoLoss: "excenv_ppo_loss_t",
           RowMoments: "excenv_row_moments_t", EpisodeStats: "excenv_episode_stats_t", Lqr: "excenv_lqr_t"}

_vp, _ci, _i32, _i64, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_STEP = [_ci, _ci, _ci, _i64, _vp, _vp, _cd, _vp, _vp, _vp, _vp]  # env, solver, dtype, B, props, control, tau, in, action, out, obs
_AHEAD = [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _vp, _ci, _vp, _vp, _ci, _vp, _ci, _vp]  # ... semantics, gym
# every function include/excenv.h declares: (restype, argtypes). Every pointer is a void*: structures go in as byref(), arrays as
# ctypes arrays, device addresses as plain ints.
PROTOTYPES = {
    "excenv_abi_version": (_ci, []),
    "excenv_last_error": (ctypes.c_char_p, []),
    "excenv_last_launch": (ctypes.c_char_p, []),
    "excenv_env_dims": (_ci, [_ci, _vp, _vp, _vp, _vp]),
    "excenv_step_bytes": (_i64, [_ci, _ci]),
    "excenv_sim_ahead_bytes": (_i64, [_ci, _ci, _ci]),
    "excenv_step": (_ci, _STEP + [_vp, _vp]),
    "excenv_truncated_width": (_i32, [_ci, _i32]),
    "excenv_gym_step": (_ci, _STEP + [_vp, _vp, _vp, _vp, _vp]),
    "excenv_sim_ahead": (_ci, _AHEAD + [_vp, _vp]),
    "excenv_sim_ahead_workspace_bytes": (_i64, [_ci, _ci, _i64, _i64, _i32, _i32, _ci, _ci, _ci]),
    "excenv_sim_ahead_ws": (_ci, _AHEAD + [_vp, _i64, _vp, _vp]),
    "excenv_sim_ahead_fuses_actions": (_ci, [_ci, _ci, _ci, _i64, _i64, _vp, _i32, _ci, _ci, _ci, _vp, _vp]),
    "excenv_sim_ahead_vjp_workspace_bytes": (_i64, [_ci, _ci, _i64, _i64, _ci]),
    "excenv_sim_ahead_vjp_workspace_bytes_for": (_i64, [_ci, _ci, _ci, _i64, _i64, _i32, _ci, _ci]),
    # ... props, control, obs_stepsize, env_tau, actions, layout, state_traj, grad_obs, grad_states, grad_last, grad_actions,
    # grad_state_in, semantics, workspace, workspace_bytes, opts, stream
    "excenv_sim_ahead_vjp": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci,
                                   _vp, _i64, _vp, _vp]),
    # the same, then grad_params (behind `stream`: the C order)
    "excenv_sim_ahead_vjp_params": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _ci, _vp, _i64, _vp, _vp, _vp]),
    "excenv_param_differentiable": (_ci, [_ci, _ci]),
    "excenv_param_grad_sum_workspace_bytes": (_i64, [_ci, _i64, _i32]),
    "excenv_param_grad_sum": (_ci, [_ci, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    "excenv_transpose": (_ci, [_ci, _i64, _i64, _vp, _vp, _vp]),
    "excenv_rew_trunc_term": (_ci, [_ci, _ci, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _ci, _vp]),
    "excenv_rew_reads": (_ci, [_ci, _i32, _vp, _vp]),
    # env, dtype, B, rows, props, control, ref_strides, state_traj, its two strides, grad_reward, its two strides, grad_state_traj,
    # opts, stream
    "excenv_rew_vjp": (_ci, [_ci, _ci, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    # env, solver, dtype, B, props, control, tau, state_in, action, state_out, grad_obs, grad_state_out, grad_reward, grad_state_in,
    # grad_action, opts, stream
    "excenv_step_vjp": (_ci, [_ci, _ci, _ci, _i64, _vp, _vp, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "excenv_step_vjp_bytes": (_i64, [_ci, _ci, _i32, _ci, _ci, _ci]),
    # env, solver, dtype, B, rows, substeps, props, n_control, dt, env_tau, state_in, state_out, state_row_stride, action, its three
    # strides (row, component, environment), row_kind, jacobian, opts, stream
    "excenv_step_jacobian": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _i32, _cd, _cd, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _ci,
                                   _vp, _vp, _vp]),
    "excenv_step_jacobian_bytes": (_i64, [_ci, _ci, _ci]),
    # env, solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, state_in, policy, obs_traj, state_traj, last_state,
    # actions_out, opts, stream
    "excenv_sim_feedback": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the arguments of excenv_sim_feedback, `policy` an excenv_policy_t
    "excenv_sim_policy": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the arguments of excenv_sim_policy with `episode` (an excenv_episode_t) behind actions_out
    "excenv_sim_policy_episodes": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp]),
    "excenv_sim_feedback_vjp_workspace_bytes": (_i64, [_ci, _ci, _i64, _i64, _i32, _i64, _ci]),
    "excenv_sim_feedback_vjp_bytes": (_i64, [_ci, _ci, _i32, _i32, _ci, _ci, _ci, _ci]),
    # env, solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, call, workspace, workspace_bytes, opts, stream
    "excenv_sim_feedback_vjp": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _vp, _i64, _vp, _vp]),
    # env, dtype, n_control, substeps, has_grad_obs, has_grad_states, has_grad_actions, has_reset
    "excenv_sim_policy_vjp_bytes": (_i64, [_ci, _ci, _i32, _i32, _ci, _ci, _ci, _ci]),
    # env, solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, call, opts, stream
    "excenv_sim_policy_vjp": (_ci, [_ci, _ci, _ci, _i64, _i64, _i32, _vp, _vp, _cd, _cd, _vp, _vp, _vp]),
    # dtype, B, K, policy, max_groups
    "excenv_policy_param_grad_workspace_bytes": (_i64, [_ci, _i64, _i64, _vp, _i32]),
    # dtype, B, K, substeps, call, stream
    "excenv_policy_param_grad": (_ci, [_ci, _i64, _i64, _i32, _vp, _vp]),
    # dtype, B, R, row_stride, call, stream
    "excenv_policy_eval": (_ci, [_ci, _i64, _i64, _i64, _vp, _vp]),
    # dtype, B, K, call, stream
    "excenv_gae": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    "excenv_gaussian_logp": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    # B, K, max_groups
    "excenv_ppo_loss_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "excenv_ppo_loss": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    "excenv_ppo_loss_grad": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    # B, N, n_columns, max_groups
    "excenv_row_moments_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    # dtype, B, N, call, stream
    "excenv_row_moments": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    "excenv_episode_stats_workspace_bytes": (_i64, [_i64]),
    # dtype, B, K, call, stream
    "excenv_episode_stats": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    # dtype, B, N, call, stream
    "excenv_lqr_backward": (_ci, [_ci, _i64, _i64, _vp, _vp]),
    # dtype, n_state, n_action, time_invariant, has_q, has_r, store_all, has_ff
    "excenv_lqr_backward_bytes": (_i64, [_ci, _i32, _i32, _ci, _ci, _ci, _ci, _ci]),
    "excenv_state_from_observation": (_ci, [_ci, _ci, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "excenv_update_ref": (_ci, [_ci, _ci, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "excenv_observe": (_ci, [_ci, _ci, _i64, _vp, _vp, _vp, _vp, _vp]),
    "excenv_update_ref_to": (_ci, [_ci, _ci, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "excenv_random_state": (_ci, [_ci, _ci, _i64, _vp, _vp, _vp, _vp, _vp]),
    "excenv_allgather": (_ci, [_vp, _ci, _vp, _vp, _i64, _vp]),
    "excenv_stream_pattern": (_ci, [_i32, _vp, _vp, _i32, _vp, _vp, _i64, _i64, _i32, _vp]),
    "excenv_probe_math": (_ci, [_ci, _ci, _i64, _vp, _vp, _vp]),
    "excenv_probe_div": (_ci, [_ci, _i64, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


def library_path() -> str:
    return _LIB_PATH


def lib():
    """Load libexcenv_hip.so (built in-tree by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C exciting-environments_amd/csrc). "
                "There is no CPU fallback."
            )
        l = ctypes.CDLL(_LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
        if l.excenv_abi_version() != ABI_VERSION:
            raise ImportError("libexcenv_hip.so: ABI version mismatch")
        _lib = l
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().excenv_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def last_launch() -> str:
    """excenv_last_launch(): which kernel form the last launching call of this thread enqueued: "sim_ahead_kernel (...)" and its
    siblings after a sim_ahead call, "step_kernel (V=1|V=2|V=4|general)" after a step, the reverse-mode kernels after theirs."""
    return lib().excenv_last_launch().decode("utf-8", "replace")


def dtype_id(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.float64:
        return F64
    raise TypeError(f"unsupported dtype {dtype}: the kernels compute in float32 or float64")


def _require_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what}: tensors must live on a HIP device (got {t.device}). The batched ODE kernels have no CPU fallback."
        )


# private fast accessors of torch when this build has them, the public (slower) API otherwise
_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda i: torch.cuda.current_stream(i).cuda_stream)
cuda_get_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
cuda_is_capturing = getattr(torch._C, "_cuda_isCurrentStreamCapturing", None) or torch.cuda.is_current_stream_capturing


def raw_stream(device_index: int) -> int:
    """torch's current HIP stream on the device of that index as an integer handle (hipStream_t)."""
    return _get_raw_stream(device_index)


def _raw_stream(device: torch.device) -> int:
    """raw_stream() of a torch.device (no index: the current device)."""
    return _get_raw_stream(device.index if device.index is not None else cuda_get_device())


class _on_device:
    """`with torch.cuda.device(d)` only when d is not already current (saves a few us per launch)."""

    def __init__(self, device):
        idx = device.index
        self.ctx = None if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _ref(struct):
    """byref(struct), or NULL for None (optional excenv_control_t / excenv_launch_opts_t / excenv_traj_gym_t arguments)."""
    return None if struct is None else ctypes.byref(struct)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _ptrs(tensors: Optional[Sequence[torch.Tensor]]):
    return None if tensors is None else (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def ptr_array(addresses: Sequence[int]):
    """void*[n] from raw device addresses (pre-built once per output slot on the vmap_step fast path)."""
    return (ctypes.c_void_p * len(addresses))(*addresses)


def _i32s(values: Sequence[int]):
    return (ctypes.c_int32 * len(values))(*values) if values else None


def _launch(name: str, on: torch.Tensor, what: str, *args):
    """One launching entry point (the C arguments in front of `stream`) on the current stream of the device `on` lives on."""
    _require_device(on, what)
    fn = getattr(lib(), name)
    with _on_device(on.device):
        rc = fn(*args, _raw_stream(on.device))
    if rc != 0:
        _check(rc, name)


def _launch_then(name: str, on: torch.Tensor, what: str, args, tail):
    """_launch for an entry point whose C arguments continue behind `stream`: fn(*args, stream, *tail)."""
    _require_device(on, what)
    fn = getattr(lib(), name)
    with _on_device(on.device):
        rc = fn(*args, _raw_stream(on.device), *tail)
    if rc != 0:
        _check(rc, name)


def allgather(nccl_comm: int, send: torch.Tensor, recv: torch.Tensor):
    """excenv_allgather: ncclAllGather of `send` (this rank's contiguous slice) into `recv` ([world * send.numel()]) on torch's
    current stream, through the caller's ncclComm_t handle (an integer address). The Python mirror's ObservationGatherer uses
    torch.distributed instead; this is the entry point a non-torch binder would call."""
    _require_device(send, "excenv_allgather")
    assert send.is_contiguous() and recv.is_contiguous() and send.dtype == recv.dtype
    _launch("excenv_allgather", send, "excenv_allgather", nccl_comm, dtype_id(send.dtype), send.data_ptr(), recv.data_ptr(),
            send.numel())


def step_raw(env_id, solver_id, dtype_code, B, props_ref, control_ref, tau, in_ptrs, action_ptr, out_ptrs, obs_ptr, opts_ref,
             stream, gym=None):
    """excenv_step / excenv_gym_step with every argument already in its C form (pointer arrays and byref()s cached by the
    caller). `gym` = (reward_ptr, terminated_ptr, truncated_ptr) selects excenv_gym_step. `stream` = raw_stream() of the
    device the buffers live on, which the caller has made current."""
    if gym is None:
        rc = _lib.excenv_step(env_id, solver_id, dtype_code, B, props_ref, control_ref, tau, in_ptrs, action_ptr, out_ptrs,
                              obs_ptr, opts_ref, stream)
    else:
        rc = _lib.excenv_gym_step(env_id, solver_id, dtype_code, B, props_ref, control_ref, tau, in_ptrs, action_ptr, out_ptrs,
                                  obs_ptr, gym[0], gym[1], gym[2], opts_ref, stream)
    if rc != 0:
        _check(rc, "excenv_step" if gym is None else "excenv_gym_step")


def step(env_id, solver_id, dtype, B, props: Props, control: Optional[Control], tau: float,
         state_in: Sequence[torch.Tensor], action: torch.Tensor, state_out: Sequence[torch.Tensor],
         obs: torch.Tensor, opts: Optional[LaunchOpts] = None):
    _require_device(action, "vmap_step")
    lib()
    with _on_device(action.device):
        step_raw(env_id, solver_id, dtype_id(dtype), B, ctypes.byref(props), _ref(control), tau, _ptrs(state_in),
                 action.data_ptr(), _ptrs(state_out), obs.data_ptr(), _ref(opts), _raw_stream(action.device))


def sim_ahead_raw(env_id, solver_id, dtype_code, B, K, substeps, props_ref, control_ref, obs_stepsize, env_tau, in_ptrs,
                  actions_ptr, action_layout, obs_ptr, traj_ptrs, traj_layout, last_ptrs, semantics, ws_ptr, ws_bytes, opts_ref,
                  stream, gym_ref=None):
    """excenv_sim_ahead_ws with every argument already in its C form (what vmap_sim_ahead calls; gym_ref: None or
    byref(TrajGym)). The caller has made the buffers' device current."""
    rc = _lib.excenv_sim_ahead_ws(env_id, solver_id, dtype_code, B, K, substeps, props_ref, control_ref, obs_stepsize, env_tau,
                                  in_ptrs, actions_ptr, action_layout, obs_ptr, traj_ptrs, traj_layout, last_ptrs, semantics,
                                  gym_ref, ws_ptr, ws_bytes, opts_ref, stream)
    if rc != 0:
        _check(rc, "excenv_sim_ahead")


def sim_ahead(env_id, solver_id, dtype, B, K, substeps, props: Props, control: Optional[Control],
              obs_stepsize: float, env_tau: float, state_in: Sequence[torch.Tensor], actions: torch.Tensor,
              action_layout: int, obs_traj: torch.Tensor, state_traj: Optional[Sequence[torch.Tensor]],
              traj_layout: int, last_state: Sequence[torch.Tensor], semantics: int,
              workspace: Optional[torch.Tensor] = None, opts: Optional[LaunchOpts] = None, gym=None):
    """sim_ahead_raw for tensors. gym: None or (reward, terminated, truncated) device tensors in the trajectory layout
    (excenv_traj_gym_t)."""
    _require_device(obs_traj, "vmap_sim_ahead")
    g = None if gym is None else TrajGym(*[t.data_ptr() for t in gym])
    lib()
    with _on_device(obs_traj.device):
        sim_ahead_raw(env_id, solver_id, dtype_id(dtype), B, K, substeps, ctypes.byref(props), _ref(control), obs_stepsize,
                      env_tau, _ptrs(state_in), actions.data_ptr() if K > 0 else None, action_layout, obs_traj.data_ptr(),
                      _ptrs(state_traj), traj_layout, _ptrs(last_state), semantics, _ptr(workspace),
                      workspace.numel() * workspace.element_size() if workspace is not None else 0, _ref(opts),
                      _raw_stream(obs_traj.device), _ref(g))


def stream_pattern(read_ptrs, read_row_strides, write_ptrs, write_row_strides, row_bytes: int, rows: int, stream: int,
                   nontemporal: bool = True):
    """excenv_stream_pattern: the trajectory kernels' access shape without arithmetic over raw device addresses (calibration;
    whatever the write streams point at is overwritten with meaningless values)."""
    nr, nw = len(read_ptrs), len(write_ptrs)
    rc = lib().excenv_stream_pattern(
        nr, (ctypes.c_void_p * max(nr, 1))(*read_ptrs), (ctypes.c_int64 * max(nr, 1))(*read_row_strides),
        nw, (ctypes.c_void_p * max(nw, 1))(*write_ptrs), (ctypes.c_int64 * max(nw, 1))(*write_row_strides),
        int(row_bytes), int(rows), int(bool(nontemporal)), stream)
    if rc != 0:
        _check(rc, "excenv_stream_pattern")


_hip = None


def _hip_runtime():
    """The HIP runtime torch already loaded (only hipMalloc / hipFree are used: spacer allocations that must not go through
    torch's caching allocator, core_env.py trajectory placement)."""
    global _hip
    if _hip is None:
        # the very file this process has mapped (torch ships its own copy): opening another copy would start a second runtime
        loaded = None
        try:
            with open("/proc/self/maps") as f:
                for line in f:
                    if "libamdhip64" in line:
                        loaded = line.split()[-1]
                        break
        except OSError:
            loaded = None
        for name in ([loaded] if loaded else []):
            try:
                h = ctypes.CDLL(name)
                h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
                h.hipMalloc.restype = ctypes.c_int
                h.hipFree.argtypes = [ctypes.c_void_p]
                h.hipFree.restype = ctypes.c_int
                _hip = h
                break
            except OSError:
                continue
        if _hip is None:
            _hip = False
    return _hip or None


def raw_malloc(nbytes: int):
    """hipMalloc outside torch's allocator; None when it fails (out of memory) or the runtime cannot be reached."""
    h = _hip_runtime()
    if h is None:
        return None
    p = ctypes.c_void_p()
    if h.hipMalloc(ctypes.byref(p), int(nbytes)) != 0 or not p.value:
        return None
    return p.value


def raw_free(ptr):
    h = _hip_runtime()
    if h is not None and ptr:
        h.hipFree(ptr)


def env_dims(env_id: int):
    dims = (ctypes.c_int32 * 4)()  # S, A, O, P
    _check(lib().excenv_env_dims(env_id, *[ctypes.byref(dims, 4 * i) for i in range(4)]), "excenv_env_dims")
    return tuple(dims)


def step_bytes(env_id: int, dtype: torch.dtype) -> int:
    return lib().excenv_step_bytes(env_id, dtype_id(dtype))


def sim_ahead_bytes(env_id: int, dtype: torch.dtype, with_state_traj: bool = True) -> int:
    return lib().excenv_sim_ahead_bytes(env_id, dtype_id(dtype), int(with_state_traj))


def truncated_width(env_id: int, n_control: int) -> int:
    return lib().excenv_truncated_width(env_id, n_control)


def launch_opts(envs_per_lane: int = 0, env_major_mode: int = 0, lds_pad_bytes: int = 0, flags: int = 0) -> LaunchOpts:
    return LaunchOpts(int(envs_per_lane), int(env_major_mode), int(lds_pad_bytes), int(flags))


def sim_ahead_fuses_actions(env: int, solver: int, dtype: torch.dtype, B: int, K: int, props, n_control: int, with_gym: bool,
                            action_layout: int, traj_layout: int, actions_ptr: int, opts: Optional[LaunchOpts]) -> bool:
    """excenv_sim_ahead_fuses_actions: the trajectory kernel reads these row-major actions itself (no workspace needed)."""
    return bool(lib().excenv_sim_ahead_fuses_actions(env, solver, dtype_id(dtype), B, K, ctypes.byref(props), n_control, int(with_gym),
                                                     action_layout, traj_layout, actions_ptr, _ref(opts)))


def sim_ahead_workspace_bytes(env_id, dtype, B, K, substeps, n_control, action_layout, traj_layout,
                              with_state_traj=True) -> int:
    return lib().excenv_sim_ahead_workspace_bytes(env_id, dtype_id(dtype), B, K, substeps, n_control, action_layout, traj_layout,
                                                  int(with_state_traj))


def make_control(control_idx: Sequence[int], refs: Sequence[torch.Tensor],
                 obs_refs: Optional[Sequence[torch.Tensor]] = None) -> Optional[Control]:
    if not control_idx:
        return None
    c = Control()
    c.n_control = len(control_idx)
    for j, (f, r) in enumerate(zip(control_idx, refs)):
        c.control_idx[j] = f
        c.reference[j] = r.data_ptr()
        if obs_refs is not None:
            c.obs_reference[j] = obs_refs[j].data_ptr()
    return c


def rew_trunc_term(env_id, dtype, B, rows, props: Props, control: Optional[Control], ref_strides: Optional[Sequence[int]],
                   state_traj: Sequence[torch.Tensor], s_sb: int, s_sk: int, reward: torch.Tensor, terminated: torch.Tensor,
                   truncated: torch.Tensor, out_layout: int):
    """excenv_rew_trunc_term: reward / terminated / truncated of a stored trajectory (one thread per (env, row))."""
    rs = (ctypes.c_int64 * len(ref_strides))(*ref_strides) if ref_strides else None
    _launch("excenv_rew_trunc_term", truncated, "vmap_generate_rew_trunc_term_ahead", env_id, dtype_id(dtype), B, rows,
            ctypes.byref(props), _ref(control), rs, _ptrs(state_traj), s_sb, s_sk, reward.data_ptr() if rows > 1 else None,
            terminated.data_ptr() if rows > 1 else None, truncated.data_ptr(), out_layout)


def rew_reads(env_id, control_idx: Sequence[int]):
    """excenv_rew_reads: [bool] per state leaf (MAX_STATE entries) — does the reward with these controlled fields read it?"""
    reads = (ctypes.c_uint8 * MAX_STATE)()
    _check(lib().excenv_rew_reads(env_id, len(control_idx), _i32s(control_idx), reads), "excenv_rew_reads")
    return [bool(r) for r in reads]


def rew_vjp(env_id, dtype, B, rows, props: Props, control: Optional[Control], ref_strides: Optional[Sequence[int]],
            state_traj: Sequence[torch.Tensor], s_sb: int, s_sk: int, grad_reward: Optional[torch.Tensor], g_sb: int, g_sk: int,
            grad_state_traj: Sequence[Optional[torch.Tensor]], opts: Optional[LaunchOpts] = None):
    """excenv_rew_vjp: the transposed reward of a stored trajectory; grad_state_traj holds a lane-major [rows, B] tensor per leaf
    the reward reads (None elsewhere)."""
    rs = (ctypes.c_int64 * len(ref_strides))(*ref_strides) if ref_strides else None
    outs = (ctypes.c_void_p * len(grad_state_traj))(*[None if t is None else t.data_ptr() for t in grad_state_traj])
    _launch("excenv_rew_vjp", state_traj[0], "vmap_reward_vjp", env_id, dtype_id(dtype), B, rows, ctypes.byref(props), _ref(control),
            rs, _ptrs(state_traj), s_sb, s_sk, _ptr(grad_reward) if rows > 1 else None, g_sb, g_sk, outs, _ref(opts))


def step_vjp_bytes(env_id: int, dtype: torch.dtype, n_control: int = 0, grad_obs: bool = True, grad_state: bool = True,
                   grad_reward: bool = False) -> int:
    """excenv_step_vjp_bytes: the algorithmic bytes per environment of one excenv_step_vjp launch with these cotangent groups."""
    return lib().excenv_step_vjp_bytes(env_id, dtype_id(dtype), n_control, int(grad_obs), int(grad_state), int(grad_reward))


def step_jacobian_bytes(env_id: int, dtype: torch.dtype, rows: str = "state") -> int:
    """excenv_step_jacobian_bytes: the algorithmic bytes per step instance of one excenv_step_jacobian launch."""
    return lib().excenv_step_jacobian_bytes(env_id, dtype_id(dtype), JAC_ROWS[rows])


def state_from_observation(env_id, dtype, B, props: Props, control_idx: Sequence[int], obs: torch.Tensor,
                           state_out: Sequence[torch.Tensor], reference_out: Sequence[torch.Tensor]):
    """excenv_state_from_observation: obs [B, O + n_control] -> denormalised state leaves (+ controlled reference leaves)."""
    nc = len(control_idx)
    _launch("excenv_state_from_observation", obs, "vmap_generate_state_from_observation", env_id, dtype_id(dtype), B,
            ctypes.byref(props), nc, _i32s(control_idx), obs.data_ptr(), _ptrs(state_out), _ptrs(reference_out) if nc else None)


def update_ref(env_id, dtype, B, props: Props, control_idx: Sequence[int], reference: Sequence[torch.Tensor],
               keys: torch.Tensor, hold: torch.Tensor, hold_min: int, hold_max: int):
    """excenv_update_ref: in-place reference redraw + hold countdown (GymWrapper.update_ref). keys: int64 [B, 2], hold: int64 [B]."""
    _require_device(keys, "GymWrapper.update_ref")
    assert keys.dtype == torch.int64 and keys.is_contiguous() and hold.dtype == torch.int64 and hold.is_contiguous()
    nc = len(control_idx)
    _launch("excenv_update_ref", keys, "GymWrapper.update_ref", env_id, dtype_id(dtype), B, ctypes.byref(props), nc,
            _i32s(control_idx), _ptrs(reference) if nc else None, keys.data_ptr(), hold.data_ptr(), hold_min, hold_max)


def observe(env_id, dtype, B, props: Props, control: Optional[Control], state: Sequence[torch.Tensor], obs: torch.Tensor):
    """excenv_observe: generate_observation for a batch of states in one launch (obs: [B, O + n_control] row-major)."""
    _launch("excenv_observe", obs, "generate_observation", env_id, dtype_id(dtype), B, ctypes.byref(props), _ref(control),
            _ptrs(state), obs.data_ptr())


def update_ref_to(env_id, dtype, B, props: Props, control_idx: Sequence[int], reference_in: Sequence[torch.Tensor],
                  keys_in: torch.Tensor, hold_in: torch.Tensor, reference_out: Sequence[torch.Tensor], keys_out: torch.Tensor,
                  hold_out: torch.Tensor, hold_min: int, hold_max: int):
    """excenv_update_ref_to: out-of-place reference redraw + hold countdown (inputs untouched, one launch, no copies)."""
    _require_device(keys_in, "GymWrapper.update_ref")
    for t in (keys_in, hold_in, keys_out, hold_out):
        assert t.dtype == torch.int64 and t.is_contiguous()
    nc = len(control_idx)
    _launch("excenv_update_ref_to", keys_in, "GymWrapper.update_ref", env_id, dtype_id(dtype), B, ctypes.byref(props), nc,
            _i32s(control_idx), _ptrs(reference_in) if nc else None, keys_in.data_ptr(), hold_in.data_ptr(),
            _ptrs(reference_out) if nc else None, keys_out.data_ptr(), hold_out.data_ptr(), hold_min, hold_max)


def random_state(env_id, dtype, B, props: Props, keys: torch.Tensor, state_out: Sequence[torch.Tensor], key_leaf: torch.Tensor):
    """excenv_random_state: init_state(key) for every environment in one launch (keys / key_leaf: int64 [B, 2])."""
    _require_device(keys, "vmap_init_state")
    assert keys.dtype == torch.int64 and keys.is_contiguous() and key_leaf.dtype == torch.int64 and key_leaf.is_contiguous()
    _launch("excenv_random_state", keys, "vmap_init_state", env_id, dtype_id(dtype), B, ctypes.byref(props), keys.data_ptr(),
            _ptrs(state_out), key_leaf.data_ptr())


def transpose(x: torch.Tensor) -> torch.Tensor:
    """out[n][m] = in[m][n] for a contiguous 2-D device tensor (the library's LDS-tiled conversion kernel)."""
    _require_device(x, "transpose")
    assert x.ndim == 2 and x.is_contiguous()
    out = torch.empty((x.shape[1], x.shape[0]), dtype=x.dtype, device=x.device)
    _launch("excenv_transpose", x, "transpose", dtype_id(x.dtype), x.shape[0], x.shape[1], x.data_ptr(), out.data_ptr())
    return out


def probe_math(which: int, x: torch.Tensor) -> torch.Tensor:
    _require_device(x, "probe_math")
    x = x.contiguous()
    out = torch.empty_like(x)
    _launch("excenv_probe_math", x, "probe_math", which, dtype_id(x.dtype), x.numel(), x.data_ptr(), out.data_ptr())
    return out


def probe_div(num: torch.Tensor, den: torch.Tensor):
    """(InvDiv(den).div(num), num / den) element-wise on the device (tests: equal bits)."""
    _require_device(num, "probe_div")
    num, den = num.contiguous(), den.contiguous()
    assert num.shape == den.shape and num.dtype == den.dtype
    fast, ref = torch.empty_like(num), torch.empty_like(num)
    _launch("excenv_probe_div", num, "probe_div", dtype_id(num.dtype), num.numel(), num.data_ptr(), den.data_ptr(),
            fast.data_ptr(), ref.data_ptr())
    return fast, ref
