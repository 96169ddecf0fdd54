"""Reverse mode of `vmap_step` / `vmap_gym_step`: the explicit vector-Jacobian product `vmap_step_vjp` (one launch of
step_vjp_kernel through `excenv_step_vjp`, include/excenv.h) and the `torch.autograd.Function` both methods go through when
`env.differentiable` is set and the action or a physical-state leaf asks for a gradient — the closed loop, where the action of step
n is `policy(obs_n)` and the gradient of the accumulated reward flows through every step. Mixed into `CoreEnvironment` (core_env.py).

The kernel reads the step's two states as [B] leaves, the action row-major as `vmap_step` took it and the cotangents as autograd
hands them over: `obs` row-major [B, obs_dim], [B] state leaves, the reward [B, 1]. Nothing is transposed; a cotangent that is not
contiguous (an expanded scalar after `sum()`) is materialised once. Gradients w.r.t. the static parameters, the references and the
normalisation bounds are not computed here (DESIGN.md §4.9 "Step")."""
from __future__ import annotations

import ctypes
from dataclasses import replace

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._reverse import _leaf_list, cotangent, count_control, opt_ptrs, unsupported


class _Step(torch.autograd.Function):
    """vmap_step (gym False) / vmap_gym_step (gym True) with a graph behind the outputs: (action, physical-state leaves) ->
    (obs, [reward, terminated, truncated,] new physical-state leaves). Forward is the launch both methods always make; saves the
    action, the incoming and the outgoing leaves and the references of the controlled fields; backward is one excenv_step_vjp launch."""

    @staticmethod
    def forward(ctx, env, state, gym, action, *leaves):
        ctx.set_materialize_grads(False)
        B = env.batch_size
        plain = [env._t(l.detach(), (B,)) for l in leaves]
        st = replace(state, physical_state=env.PhysicalState(*plain))
        ctx.packed = env._props_for(env.env_properties, B)  # the values of this forward, whatever happens to the leaves later
        out = env._vmap_step_launch(st, action.detach(), gym)
        # aliases of the slot's tensors: the pool's own tensor objects never carry a grad_fn, and a live graph keeps the slot busy
        # through them (StepSlotPool hands a slot out again only when nothing refers to its memory)
        new_leaves = [getattr(out[-1].physical_state, n).detach() for n in env.STATE_FIELDS]
        refs = [env._t(getattr(state.reference, n), (B,)).detach() for n in env.control_state] if gym else []
        if gym:
            outs = (out[0].detach(), out[1].detach(), out[2].detach(), out[3].detach()) + tuple(new_leaves)
            ctx.mark_non_differentiable(outs[2], outs[3])
        else:
            outs = (out[0].detach(),) + tuple(new_leaves)
        ctx.env, ctx.gym, ctx.S = env, gym, len(plain)
        ctx.save_for_backward(action, *plain, *new_leaves, *refs)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, *g):
        env, S = ctx.env, ctx.S
        action, *saved = ctx.saved_tensors
        st_in, st_out, refs = saved[:S], saved[S:2 * S], saved[2 * S:]
        g_rew = g[0] if ctx.gym else None
        g_state = list(g[3:] if ctx.gym else g)
        need = ctx.needs_input_grad
        if g_obs is None and g_rew is None and all(t is None for t in g_state):
            return (None,) * (4 + S)
        ga, gs = env._step_vjp_launch(st_in, action, st_out, g_obs, g_state if any(t is not None for t in g_state) else None,
                                      g_rew, refs=refs, packed=ctx.packed)
        return (None, None, None, ga if need[3] else None) + tuple(t if n else None for t, n in zip(gs, need[4:4 + S]))


class StepVjpMixin:
    # excenv_last_launch() of the most recent excenv_step_vjp launch, read on the thread that enqueued it (autograd runs backward on a
    # thread of its own), and which cotangent groups that launch was handed: {"obs": bool, "state": [bool per leaf], "reward": bool}
    last_step_vjp_launch = ""
    last_step_vjp_cotangents = None

    def _step_wants_grad(self, state, action):
        """env.differentiable is set (the caller has looked): grad mode on and the action or a physical-state leaf requires grad"""
        if not torch.is_grad_enabled():
            return False
        if action.requires_grad:
            return True
        ps = state.physical_state
        return any(isinstance(t, torch.Tensor) and t.requires_grad for t in (getattr(ps, n) for n in self.STATE_FIELDS))

    def _step_vjp_unsupported(self):
        """The reason this environment's configuration has no reverse-mode step, or None."""
        return unsupported(self)

    def _step_differentiable(self, state, action, gym: bool):
        what = "vmap_gym_step" if gym else "vmap_step"
        why = self._step_vjp_unsupported()
        if why is not None:
            raise ValueError(f"{what}(differentiable): {why}")
        params = self._param_leaves()
        if params:
            names = ", ".join(repr(self.PARAM_FIELDS[j]) for j, _ in params)
            raise ValueError(f"{what}(differentiable): static parameter {names} requires grad, and a step has no parameter gradients "
                             "(use vmap_sim_ahead, or detach the parameter)")
        B = self.batch_size
        if action.device != self.device or action.dtype != self.dtype:
            action = action.to(device=self.device, dtype=self.dtype)
        leaves = [torch.as_tensor(getattr(state.physical_state, n)) for n in self.STATE_FIELDS]
        assert tuple(leaves[0].shape) + (len(leaves),) == (B, self.physical_state_dim), (
            "The physical state needs to be of shape (batch_size, physical_state_dim) which is "
            + f"{(B, self.physical_state_dim)}, but {tuple(leaves[0].shape) + (len(leaves),)} is given"
        )
        outs = _Step.apply(self, state, gym, action, *leaves)
        n0 = 4 if gym else 1
        add = self._active_additions
        if add is None:
            add = self._active_additions = self._additions((B,), True)
        new_state = self.State(self.PhysicalState(*outs[n0:]), state.PRNGKey, add, state.reference)
        return tuple(outs[:n0]) + (new_state,)

    # ------------------------------------------------------------------ the explicit form
    def vmap_step_vjp(self, state, action, new_state, grad_obs=None, grad_state=None, grad_reward=None):
        """Vector-Jacobian product of `obs, new_state = vmap_step(state, action)` and, with grad_reward, of the reward of
        `vmap_gym_step(state, action)`. new_state: the state that call returned (read, not recomputed). grad_obs [B, obs_dim]
        (columns of controlled references are ignored), grad_state (a State / PhysicalState pytree or a sequence of [B] leaves,
        None where absent), grad_reward [B, 1] or [B]: the cotangents, any of them may be None.
        Returns (grad_action [B, A], PhysicalState of [B] gradients w.r.t. `state.physical_state`). Works whatever
        `env.differentiable` says. Derivatives of clamps / clips are 0 on the boundary, of sign 0, and the reward's are those of
        `vmap_reward_vjp`; static parameters, references and normalisation bounds get no gradient."""
        why = self._step_vjp_unsupported()
        if why is not None:
            raise ValueError(f"vmap_step_vjp: {why}")
        B = self.batch_size
        st_in = [self._t(l, (B,)) for l in _leaf_list(state, self.STATE_FIELDS)]
        st_out = [self._t(l, (B,)) for l in _leaf_list(new_state, self.STATE_FIELDS)]
        refs = [self._t(getattr(state.reference, n), (B,)) for n in self.control_state] if grad_reward is not None else []
        g_state = _leaf_list(grad_state, self.STATE_FIELDS)
        if g_state is not None and all(g is None for g in g_state):
            g_state = None
        ga, gs = self._step_vjp_launch(st_in, torch.as_tensor(action), st_out, grad_obs, g_state, grad_reward, refs=refs)
        return ga, self.PhysicalState(*gs)

    def _step_vjp_launch(self, st_in, action, st_out, g_obs, g_state, g_reward, refs=(), packed=None):
        """-> (grad_action [B, A], [grad of the incoming state leaves]): one excenv_step_vjp launch, one allocation.
        st_in / st_out: [B] leaves of the working dtype on the device; refs: the [B] references of control_state (read with a reward
        cotangent); packed: the forward's packed properties."""
        B, S, A, OW = self.batch_size, self.physical_state_dim, self.action_dim, self._obs_dim()
        dt, dev = self.dtype, self.device
        action = self._t(action.detach(), (B, A))
        if action.data_ptr() % 16:  # a contiguous slice that starts inside a 16-byte piece: rows are read as 16-byte pieces
            action = action.clone()
        if g_obs is not None:  # rows are read as 16-byte pieces; the [B] cotangents are read one element per lane
            g_obs = cotangent(g_obs, dev, dt, (B, OW))
        if g_state is not None:
            g_state = [None if g is None else cotangent(g, dev, dt, (B,), align=False) for g in g_state]
        if g_reward is not None and not self.control_state:
            g_reward = None  # without controlled fields the reward is a constant
        g_reward = None if g_reward is None else cotangent(g_reward, dev, dt, (B,), align=False)
        props, _keep = packed if packed is not None else self._props_for(self.env_properties, B)
        if g_reward is not None:  # set with controlled fields only
            control = _native.make_control([self.STATE_FIELDS.index(n) for n in self.control_state], list(refs))
        else:
            control = count_control(self)
        al = 16 // (4 if dt == torch.float32 else 8)
        Bp = (B + al - 1) // al * al  # every leaf and the action block 16-byte aligned inside the single allocation
        buf = torch.empty(S * Bp + B * A, dtype=dt, device=dev)
        gs = [buf[j * Bp: j * Bp + B] for j in range(S)]
        ga = buf[S * Bp:].view(B, A)
        self.last_step_vjp_cotangents = {"obs": g_obs is not None,
                                         "state": [False] * S if g_state is None else [g is not None for g in g_state],
                                         "reward": g_reward is not None}
        _native._launch("excenv_step_vjp", buf, "vmap_step_vjp", self.ENV_ID, self._solver.id, _native.dtype_id(dt), B,
                        ctypes.byref(props), _native._ref(control), float(self.tau), _native._ptrs(st_in), action.data_ptr(),
                        _native._ptrs(st_out), _native._ptr(g_obs), opt_ptrs(g_state), _native._ptr(g_reward), _native._ptrs(gs),
                        ga.data_ptr(), _native._ref(self.launch_opts))
        self.last_step_vjp_launch = _native.last_launch()
        return ga, gs
