"""Closed-loop trajectories: `vmap_sim_ahead_feedback` runs a whole horizon in ONE persistent launch of sim_feedback_kernel through
`excenv_sim_feedback` (include/excenv.h), with every action computed inside the kernel from the observation row it has just saved:
affine output feedback, optional integral action, optional feedforward row. Mixed into `CoreEnvironment`
(core_env.py); what it shares with `vmap_sim_ahead_policy` is _closed_loop.py's. Nothing here records a graph: the reverse mode
through the policy is _feedback_vjp.py's, asked for with `differentiable=True`."""
from __future__ import annotations

import torch

from . import _closed_loop, _native


class FeedbackMixin:
    # excenv_last_launch() of the most recent excenv_sim_feedback launch of this environment
    last_feedback_launch = ""

    def _lane_major_gain(self, gain, what):
        """[A, OW] (one gain set for all) or [B, A, OW] (one per environment) -> (tensor over [A][OW][Bg] memory, Bg)"""
        B, A, OW = self.batch_size, self.action_dim, self._obs_dim()
        gain = torch.as_tensor(gain).detach()
        assert tuple(gain.shape) in ((A, OW), (B, A, OW)), (
            f"{what} needs to be of shape (action_dim, obs_dim) or (batch_size, action_dim, obs_dim) which is {(A, OW)} or "
            f"{(B, A, OW)}, but {tuple(gain.shape)} is given")
        if gain.device != self.device or gain.dtype != self.dtype:
            gain = gain.to(device=self.device, dtype=self.dtype)
        if gain.ndim == 2:
            return gain.contiguous(), 1
        if B > 0 and tuple(gain.stride()) != (1, OW * B, B):
            gain = gain.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        return gain, B

    def vmap_sim_ahead_feedback(self, init_state, gain, n_actions, obs_stepsize, action_stepsize, feedforward=None,
                                integral_gain=None, integrator_state=None, clip=(-1.0, 1.0), differentiable=None):
        """Closed-loop trajectories of all batch_size environments in one kernel launch -> (observations [B, N+1, OW],
        states with leaves [B, N+1], last_state with leaves [B], actions [B, K, A], z [B, A] or None), K = n_actions action rows
        of substeps = action_stepsize / obs_stepsize solver steps each, N = K * substeps.

        At every action row k the kernel reads the observation row it has just saved (row k * substeps, the normalised references
        of `control_state` included: what `generate_observation` builds) and applies, per action component q,
            a[k, q] = clamp(feedforward[k, q] + z[q] + sum_o gain[q, o] * obs[o])
            z[q]    = clamp(z[q] + action_stepsize * sum_o integral_gain[q, o] * obs[o])
        (sums as fused multiply-adds in column order; z only with `integral_gain`, its clamp is the anti-windup). The normalised
        action is held for `substeps` steps of `vmap_step`'s arithmetic.

        gain, integral_gain: [A, OW] (one gain set for every environment) or [B, A, OW] (one per environment).
        feedforward: [B, K, A] or None; a view from `env.new_actions_buffer(K)` is read in place, anything else is copied into one.
        n_actions: K; may be None when `feedforward` gives it. integrator_state: the initial z [B, A] (None: zeros).
        clip: (low, high) for both clamps, None: no clamp. References of the controlled fields come from `init_state.reference`.

        The returned tensors are views of freshly allocated lane-major memory; `states` is None with
        `env.store_state_trajectory = False`. `vmap_generate_rew_trunc_term_ahead(states, actions)` gives the gym outputs.
        Refused by name (ValueError): trajectory layouts other than "lane_major", `sim_ahead_semantics ==
        "ahead_accumulated_t"`, and (differentiable=None, the default) `env.differentiable` with an input that requires grad: the
        outputs carry no graph.

        differentiable=True: when grad mode is on and the gain, the integral gain, the feedforward, the integrator state or a leaf
        of the initial physical state requires grad, the call records ONE autograd node (_feedback_vjp.py) whose backward is one
        `vmap_sim_ahead_feedback_vjp` call; observations, state leaves, last state, actions and z carry the graph, so a loss through
        `vmap_generate_rew_trunc_term_ahead(states, actions)` under `env.differentiable` reaches `gain.grad`. With no input that
        requires grad the plain path runs. Refused then: `store_state_trajectory = False`, static parameters that require grad, the
        saturated PMSM, per-environment properties, graph capture."""
        _closed_loop.refuse_settings(self, "vmap_sim_ahead_feedback", "closed-loop")
        tensors = [gain, integral_gain, feedforward, integrator_state]
        tensors += [getattr(init_state.physical_state, n) for n in self.STATE_FIELDS]
        wants = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)
        if differentiable:
            if wants or (torch.is_grad_enabled() and self._param_leaves()):
                return self._feedback_differentiable(init_state, gain, n_actions, obs_stepsize, action_stepsize, feedforward,
                                                     integral_gain, integrator_state, clip)
        elif self.differentiable and torch.is_grad_enabled() and (self._param_leaves() or wants):
            raise ValueError("vmap_sim_ahead_feedback: env.differentiable with an input that requires grad: there is no reverse mode "
                             "through the policy; detach the inputs or set env.differentiable = False, or pass differentiable=True, "
                             "which records the closed loop's own reverse mode (vmap_sim_ahead_feedback_vjp)")
        return self._feedback_launch(init_state, gain, n_actions, obs_stepsize, action_stepsize, feedforward, integral_gain,
                                     integrator_state, clip)

    def _feedback_launch(self, init_state, gain, n_actions, obs_stepsize, action_stepsize, feedforward, integral_gain,
                         integrator_state, clip):
        """The one excenv_sim_feedback launch behind vmap_sim_ahead_feedback (its arguments, its return value); records no graph."""
        B, A, OW = self.batch_size, self.action_dim, self._obs_dim()
        _closed_loop.check_state(self, init_state, obs_stepsize, action_stepsize)
        feedforward, K = _closed_loop.action_rows(self, feedforward, "feedforward", n_actions)
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        lo, hi = _closed_loop.clip_bounds(clip)
        g, Bg = self._lane_major_gain(gain, "The gain")
        gi = None
        if integral_gain is not None:
            gi, Bgi = self._lane_major_gain(integral_gain, "The integral gain")
            if Bgi != Bg:  # one gain_batch for both: the broadcast one is repeated
                if Bg == 1:
                    g, Bg = g[:, :, None].expand(A, OW, B).contiguous().permute(2, 0, 1), B
                else:
                    gi = gi[:, :, None].expand(A, OW, B).contiguous().permute(2, 0, 1)
        z_in = None
        if integrator_state is not None:
            assert integral_gain is not None, "integrator_state without integral_gain"
            z_in = torch.as_tensor(integrator_state).detach()
            assert tuple(z_in.shape) == (B, A), (
                f"The integrator state needs to be of shape (batch_size, action_dim) which is {(B, A)}, but {tuple(z_in.shape)} is given")
            z_in = z_in.to(device=self.device, dtype=self.dtype).t().contiguous()  # [A][B]
        feedforward = _closed_loop.lane_major_rows(self, feedforward, K)
        z_buf = torch.empty((A, B), dtype=self.dtype, device=self.device) if gi is not None else None
        policy = _native.Feedback(g.data_ptr(), _native._ptr(gi), Bg, _native._ptr(feedforward) if K > 0 else None,
                                  _native._ptr(z_in), _native._ptr(z_buf), lo, hi)
        out, name = _closed_loop.launch(self, "excenv_sim_feedback", policy, "vmap_sim_ahead_feedback", init_state, K, sub, obs_stepsize)
        if name is not None:
            self.last_feedback_launch = name
        return (*out, (z_buf.t() if z_buf is not None else None))
