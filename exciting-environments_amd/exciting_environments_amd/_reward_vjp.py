"""Reverse mode of the trajectory reward: the explicit vector-Jacobian product `vmap_reward_vjp` (one launch of rew_vjp_kernel
through `excenv_rew_vjp`, include/excenv.h) and the `torch.autograd.Function` that `vmap_generate_rew_trunc_term_ahead` goes through
when `env.differentiable` is set and a state leaf asks for a gradient. Mixed into `CoreEnvironment` (core_env.py).

The reward of row n reads the state of row n only, so the product is elementwise: the kernel reads the saved rows of the leaves the
reward depends on, the references and the reward cotangent, and writes one lane-major [rows, B] array per such leaf — the layout
`vmap_sim_ahead_vjp(grad_states=...)` takes without a copy. Leaves the reward does not read have no cotangent (None).
Subgradient conventions: DESIGN.md §4.9."""
from __future__ import annotations

from dataclasses import replace

import torch
from torch.autograd.function import once_differentiable

from . import _native


class _RewTruncTerm(torch.autograd.Function):
    """vmap_generate_rew_trunc_term_ahead with a graph behind the reward: physical-state leaves [B, rows] -> (reward, truncated,
    terminated). Forward is the launch of the call without a graph; saves the state leaves and the references; backward is one
    excenv_rew_vjp launch."""

    @staticmethod
    def forward(ctx, env, states, *leaves):
        ctx.set_materialize_grads(False)
        B, rows = leaves[0].shape
        plain = env._rew_leaves([l.detach() for l in leaves])
        refs = [r.detach() for r in env._rew_refs(states.reference, B, rows)]
        ctx.packed = env._props_for(env.env_properties, B)  # the values of this forward, whatever happens to the leaves later
        reward, truncated, terminated = env._rew_trunc_term_device(states, plain, packed=ctx.packed, refs=refs)
        ctx.mark_non_differentiable(truncated, terminated)
        ctx.env, ctx.n_leaves = env, len(plain)
        ctx.save_for_backward(*plain, *refs)
        return reward, truncated, terminated

    @staticmethod
    @once_differentiable
    def backward(ctx, g_reward, _g_truncated, _g_terminated):
        env, S = ctx.env, ctx.n_leaves
        none = (None, None) + (None,) * S
        if g_reward is None:
            return none
        saved = ctx.saved_tensors
        grads = env._reward_vjp_launch(list(saved[:S]), list(saved[S:]), g_reward, packed=ctx.packed)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class RewardVjpMixin:
    # excenv_last_launch() of the most recent excenv_rew_vjp launch, read on the thread that enqueued it (autograd runs backward on
    # a thread of its own: TrajectoryVjpMixin.last_vjp_launch)
    last_reward_vjp_launch = ""

    def _reward_reads(self):
        """[bool] per physical-state leaf: does the reward with this control_state read it? (excenv_rew_reads)"""
        idx = [self.STATE_FIELDS.index(n) for n in self.control_state]
        return _native.rew_reads(self.ENV_ID, idx)[:len(self.STATE_FIELDS)]

    def _reward_wants_grad(self, leaves):
        if not (self.differentiable and torch.is_grad_enabled()):
            return False
        if not any(l.requires_grad for l in leaves):
            return False
        return any(self._reward_reads())

    def _rew_trunc_term_differentiable(self, states, leaves):
        return _RewTruncTerm.apply(self, states, *leaves)

    def vmap_reward_vjp(self, states, grad_reward):
        """Vector-Jacobian product of the reward of `vmap_generate_rew_trunc_term_ahead(states, actions)`.
        states: the trajectory `states` (physical-state leaves [B, N+1], reference leaves [B] or [B, N+1]); grad_reward: the
        cotangent of the reward, [B, N, 1] or [B, N] (a tensor that is not laid out lane-major is copied once).
        Returns the model's PhysicalState: for every leaf the reward reads a [B, N+1] cotangent — a view of lane-major [N+1, B]
        memory, what `vmap_sim_ahead_vjp(grad_states=...)` consumes without a copy; row 0 is zero (the reward covers rows 1..) —,
        None for every other leaf. Works whatever `env.differentiable` says. The torque reward's derivative is that of the branch
        the forward selected (0 where none fired), |x| has derivative sign(x) (0 at 0), sqrt(i_d^2 + i_q^2) has derivative 0 at
        the origin; references and normalisation bounds get no gradient. CPU tensors go through torch autograd over the
        elementwise torch mirror."""
        leaves = [torch.as_tensor(getattr(states.physical_state, n)) for n in self.STATE_FIELDS]
        if not (leaves[0].is_cuda and leaves[0].ndim == 2 and leaves[0].shape[0] == self.batch_size):
            return self._reward_vjp_torch(states, leaves, torch.as_tensor(grad_reward))
        B, rows = leaves[0].shape
        plain = self._rew_leaves([l.detach() for l in leaves])
        refs = [r.detach() for r in self._rew_refs(states.reference, B, rows)]
        return self.PhysicalState(*self._reward_vjp_launch(plain, refs, torch.as_tensor(grad_reward)))

    def _reward_vjp_launch(self, leaves, refs, g, packed=None):
        """-> per state leaf a [B, rows] view of a lane-major [rows, B] cotangent, or None where the reward does not read the leaf.
        leaves / refs: `_rew_leaves` / `_rew_refs`; packed: the forward's packed properties."""
        B, rows = leaves[0].shape
        N = rows - 1
        reads = self._reward_reads()
        if not any(reads):
            return [None] * len(leaves)
        outs = [torch.empty((rows, B), dtype=self.dtype, device=self.device) if r else None for r in reads]
        views = [None if o is None else o.t() for o in outs]
        if B == 0:
            return views
        if g.ndim == 3:
            assert g.shape[2] == 1, f"reward cotangent of shape {tuple(g.shape)}, expected {(B, N, 1)} or {(B, N)}"
            g = g[..., 0]
        g = self._lane_major(g.detach(), (B, N), (1, B)) if N > 0 else None
        props, keep = packed if packed is not None else self._props_for(self.env_properties, B)
        control, ref_strides = self._rew_control(refs)
        s_sb, s_sk = leaves[0].stride()
        _native.rew_vjp(self.ENV_ID, self.dtype, B, rows, props, control, ref_strides, leaves, s_sb, s_sk, g, 1, B, outs,
                        self.launch_opts)
        self.last_reward_vjp_launch = _native.last_launch()
        return views

    def _reward_vjp_torch(self, states, leaves, g):
        """The same product by torch autograd over `_rew_trunc_term_torch` (CPU tensors)."""
        with torch.enable_grad():
            free = [l.detach().to(self.dtype).requires_grad_(True) for l in leaves]
            reward, _, _ = self._rew_trunc_term_torch(replace(states, physical_state=self.PhysicalState(*free)))
            if not reward.requires_grad:
                return self.PhysicalState(*[None] * len(free))
            grads = torch.autograd.grad(reward, free, grad_outputs=g.to(reward.dtype).reshape(reward.shape), allow_unused=True)
        return self.PhysicalState(*grads)
