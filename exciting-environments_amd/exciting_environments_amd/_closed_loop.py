"""What `vmap_sim_ahead_feedback` (_feedback.py) and `vmap_sim_ahead_policy` (_policy.py) share: both run a whole horizon in ONE
persistent launch whose kernel computes every action from the observation row it has just saved, and differ in
the controller record they hand over. Here: what both refuse by name, the checks on the initial state and on the additive
[B, K, A] input (the feedforward, the noise), the clamp, and the launch with its outputs.

The rows are the post-processed states `vmap_step` carries ("step" semantics), so the returned observations, states and last state are
bit for bit what `vmap_sim_ahead` returns under `sim_ahead_semantics = "step"` for the returned actions."""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native
from ._trajectory import _lane_major_leaves, _lane_major_obs


def refuse_settings(env, fn, kernel):
    """ValueError under the caller's name `fn` for the settings no closed loop has; `kernel`: how the caller names its kernel"""
    if env.traj_layout != "lane_major":
        raise ValueError(f"{fn}: traj_layout={env.traj_layout!r}: the {kernel} kernel writes the 'lane_major' layout only")
    if env.sim_ahead_semantics == "ahead_accumulated_t":
        raise ValueError(f"{fn}: sim_ahead_semantics='ahead_accumulated_t': a closed loop reads the saved row of every action, "
                         "its trajectory is a chain of steps ('step' semantics) on every setting")


def check_state(env, init_state, obs_stepsize, action_stepsize):
    B, S = env.batch_size, env.physical_state_dim
    assert obs_stepsize <= action_stepsize, "The action stepsize should be greater or equal to the observation stepsize."
    phys_shape = env._phys_shape(init_state.physical_state)
    assert phys_shape == (B, S), (
        "The initial physical state needs to be of shape (batch_size, physical_state_dim,) which is "
        + f"{(B, S)}, but {phys_shape} is given")


def action_rows(env, x, what, n_actions):
    """The shape checks of the additive input `x` [B, K, A] (`what`: "feedforward" or "noise") or None -> (x detached or None, K).
    K is `n_actions` where x is None."""
    B, A = env.batch_size, env.action_dim
    if x is not None:
        x = torch.as_tensor(x).detach()
        assert x.ndim == 3 and x.shape[0] == B and x.shape[2] == A, (
            f"The {what} needs to have three dimensions: (batch_size, n_actions, action_dim) which is "
            + f"{(B, n_actions, A)}, but {tuple(x.shape)} is given")
        assert n_actions is None or int(n_actions) == x.shape[1], (
            f"n_actions is {n_actions}, but the {what} has {x.shape[1]} action rows")
        n_actions = x.shape[1]
    assert n_actions is not None and int(n_actions) >= 0, f"n_actions is needed where no {what} gives it"
    return x, int(n_actions)


def lane_major_rows(env, x, K):
    """The checked input of action_rows over [K][A][B] memory (None stays None), behind the caller's other refusals: a view from
    `env.new_actions_buffer(K)` is taken as it is, anything else is copied into one."""
    if x is None:
        return None
    B, A = env.batch_size, env.action_dim
    if x.device != env.device or x.dtype != env.dtype:
        x = x.to(device=env.device, dtype=env.dtype)
    if K > 0 and B > 0 and tuple(x.stride()) != (1, A * B, B):
        lane_major = env.new_actions_buffer(K)
        lane_major.copy_(x)
        x = lane_major
    return x


def clip_bounds(clip):
    lo, hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
    assert lo <= hi, f"clip needs to be (low, high) with low <= high, but {clip} is given"
    return lo, hi


def launch(env, entry, record, caller, init_state, K, sub, obs_stepsize, extra=()):
    """One `entry` launch (excenv_sim_feedback, excenv_sim_policy or excenv_sim_policy_episodes) with the ctypes policy `record`, for
    `caller` -> ((observations [B, N+1, OW], states with leaves [B, N+1] or None, last_state with leaves [B], actions [B, K, A]),
    excenv_last_launch() of it or None for an empty batch). Views of freshly allocated lane-major memory. extra: the C arguments
    an entry has between `actions_out` and `opts` (the episode record)."""
    B, S, A, OW = env.batch_size, env.physical_state_dim, env.action_dim, env._obs_dim()
    dt, N = env.dtype, K * sub
    props, _keep = env._props_for(env.env_properties, B)
    st_in = [env._t(getattr(init_state.physical_state, n), (B,)).detach() for n in env.STATE_FIELDS]
    control, _refs = env._control(init_state, (B,))
    new = lambda *shape: torch.empty(shape, dtype=dt, device=env.device)
    obs_buf = new(N + 1, OW, B)
    st_buf = [new(N + 1, B) for _ in range(S)] if env.store_state_trajectory else None
    last = [new(B) for _ in range(S)]
    act_buf = new(K, A, B)
    name = None
    if B > 0:  # (an empty batch has no addresses to hand over)
        _native._launch(entry, obs_buf, caller, env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, K, sub, ctypes.byref(props),
                        _native._ref(control), float(obs_stepsize), float(env.tau), _native._ptrs(st_in), ctypes.byref(record),
                        obs_buf.data_ptr(), _native._ptrs(st_buf), _native._ptrs(last), act_buf.data_ptr() if K > 0 else None,
                        *extra, _native._ref(env.launch_opts))
        name = _native.last_launch()
    observations = _lane_major_obs(obs_buf, B, N + 1, OW)
    states = None
    if st_buf is not None:
        states = env._traj_state(init_state, [_lane_major_leaves(b, 1, B, N + 1)[0] for b in st_buf], (B,), N)
    last_state = env.State(env.PhysicalState(*last), init_state.PRNGKey, env._additions((B,), True), init_state.reference)
    return (observations, states, last_state, act_buf.permute(2, 0, 1)), name
