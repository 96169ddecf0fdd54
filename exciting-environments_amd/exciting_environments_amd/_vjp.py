"""Reverse mode of `vmap_sim_ahead`: the explicit vector-Jacobian product `vmap_sim_ahead_vjp` (one persistent launch of
sim_ahead_vjp_kernel through `excenv_sim_ahead_vjp`, include/excenv.h) and the `torch.autograd.Function` that `vmap_sim_ahead`
goes through when `env.differentiable` is set and something asks for a gradient. Mixed into `CoreEnvironment` (core_env.py).

The kernel reads the state trajectory the forward call returned (its rows are the per-step checkpoints) and lane-major
cotangents. A cotangent that is not laid out lane-major — autograd hands such tensors back after a `select` or a `sum` (an
expanded scalar, a zero-filled row-major block) — is copied into a lane-major buffer first: one strided pass over the tensor (its cost
next to the launch's: DESIGN.md §4.9).

Gradients w.r.t. the static parameters come from the same launch (`excenv_sim_ahead_vjp_params`, the PGRAD instantiations): per
environment from the kernel, their batch sum from `excenv_param_grad_sum` (two small launches, deterministic)."""
from __future__ import annotations

import ctypes
from dataclasses import replace

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._reverse import _leaf_list, cotangent, count_control, opt_ptrs, unsupported

_EM, _LM = _native.LAYOUT_ENV_MAJOR, _native.LAYOUT_LANE_MAJOR


class _SimAhead(torch.autograd.Function):
    """vmap_sim_ahead with a graph behind its outputs: (actions, initial physical-state leaves, 0-dim static-parameter leaves that
    require grad) -> (observations, state trajectory leaves, last-state leaves). Saves the actions and the state trajectory;
    backward is one reverse launch (the PGRAD one, and the batch sum behind it, only when a parameter leaf needs a gradient).
    param_idx: the positions in PARAM_FIELDS of the parameter leaves among the inputs."""

    @staticmethod
    def forward(ctx, env, init_state, obs_stepsize, action_stepsize, param_idx, actions, *tensors):
        ctx.set_materialize_grads(False)
        S = env.physical_state_dim
        leaves = tensors[:S]
        st = replace(init_state, physical_state=env.PhysicalState(*[t.detach() for t in leaves]))
        B = env.batch_size
        # tensor parameter leaves are packed now, and the reverse launch reads this packing: the values of this forward, whatever
        # an optimiser does to the leaves in between
        ctx.packed = env._props_for(env.env_properties, B)
        ctx.param_idx = param_idx
        ctx.param_meta = [(t.device, t.dtype) for t in tensors[S:]]
        obs, st_views, last, N = env._run_sim_ahead(st, actions.detach(), env.env_properties, obs_stepsize, action_stepsize, B,
                                                    packed=ctx.packed)
        # aliases of the launch's outputs: the pooled sets' own tensor objects never carry a grad_fn, and a live graph keeps the
        # set's storage busy through them (the pools hand a set out again only when nothing refers to its memory)
        outs = [obs.detach()] + [t.detach() for t in st_views] + [t.detach() for t in last]
        ctx.env, ctx.steps, ctx.N = env, (obs_stepsize, action_stepsize), N
        ctx.save_for_backward(actions, *outs[1:1 + S])
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, *g):
        env = ctx.env
        S = env.physical_state_dim
        actions, *traj = ctx.saved_tensors
        g_states, g_last = list(g[:S]), list(g[S:])
        need = ctx.needs_input_grad
        wanted = [j for j, n in zip(ctx.param_idx, need[6 + S:]) if n]
        res = env._sim_ahead_vjp_launch(traj, actions, ctx.steps[0], ctx.steps[1], g_obs,
                                        g_states if any(t is not None for t in g_states) else None,
                                        g_last if any(t is not None for t in g_last) else None,
                                        param_idx=wanted or None, packed=ctx.packed)
        ga, gs = res[0], res[1]
        gp = ()
        if ctx.param_idx:
            sums = dict(zip(wanted, env._param_grad_sum(res[2]))) if wanted else {}
            gp = tuple(None if j not in sums else sums[j].to(device=d, dtype=t) for j, (d, t) in zip(ctx.param_idx, ctx.param_meta))
        return (None, None, None, None, None, ga if need[5] else None) + tuple(t if n else None for t, n in zip(gs, need[6:6 + S])) + gp


class TrajectoryVjpMixin:
    @property
    def differentiable(self) -> bool:
        """False (default): vmap_sim_ahead returns plain tensors, exactly as without this property. True: when grad mode is on
        and the actions or a leaf of the initial physical state require grad, the call records one autograd node whose backward
        is the reverse-mode kernel (the state trajectory is always produced then; not combinable with out=,
        return_rew_trunc_term=True or anything vmap_sim_ahead_vjp rejects). The same switch makes vmap_step / vmap_gym_step
        (an action or physical-state leaf that requires grad; _step_vjp.py) and the reward of
        vmap_generate_rew_trunc_term_ahead (_reward_vjp.py) record their nodes."""
        return getattr(self, "_differentiable", False)

    @differentiable.setter
    def differentiable(self, value):
        self._differentiable = bool(value)

    def _vjp_unsupported(self):
        """The reason this environment's configuration has no reverse mode, or None."""
        if self.sim_ahead_semantics not in ("ahead", "step"):
            return f"sim_ahead_semantics={self.sim_ahead_semantics!r} has no reverse mode (use 'ahead' or 'step')"
        if self.traj_layout != "lane_major":
            return f"traj_layout={self.traj_layout!r} has no reverse mode (the 'env_major' and 'tiled' layouts are forward only)"
        return unsupported(self)

    # excenv_last_launch() of the most recent reverse launch, read on the thread that enqueued it: the C string is per thread, and
    # autograd runs backward on a thread of its own, where the caller's excenv_last_launch() still names the forward
    last_vjp_launch = ""

    def _param_leaves(self):
        """[(position in PARAM_FIELDS, leaf)] of the static parameters that are 0-dim floating tensors with requires_grad"""
        sp = self.env_properties.static_params
        out = []
        for j, n in enumerate(self.PARAM_FIELDS):
            v = getattr(sp, n)
            if isinstance(v, torch.Tensor) and v.ndim == 0 and v.is_floating_point() and v.requires_grad:
                out.append((j, v))
        return out

    def _wants_grad(self, init_state, actions):
        if not (self.differentiable and torch.is_grad_enabled()):
            return False
        if isinstance(actions, torch.Tensor) and actions.requires_grad:
            return True
        if self._param_leaves():
            return True
        return any(isinstance(t, torch.Tensor) and t.requires_grad
                   for t in (getattr(init_state.physical_state, n) for n in self.STATE_FIELDS))

    def _sim_ahead_differentiable(self, init_state, actions, obs_stepsize, action_stepsize):
        why = self._vjp_unsupported()
        if why is None and not self.store_state_trajectory:
            why = "store_state_trajectory=False: the reverse pass reads the state trajectory"
        if why is None and actions.ndim != 3:
            why = "tiled actions have no reverse mode"
        if why is not None:
            raise ValueError(f"vmap_sim_ahead(differentiable): {why}")
        B, S = self.batch_size, self.physical_state_dim
        leaves = [self._t(getattr(init_state.physical_state, n), (B,)) for n in self.STATE_FIELDS]
        if actions.device != self.device or actions.dtype != self.dtype:
            actions = actions.to(device=self.device, dtype=self.dtype)
        params = self._param_leaves()
        for j, _ in params:
            if not _native.lib().excenv_param_differentiable(self.ENV_ID, j) == 1:
                raise ValueError(f"vmap_sim_ahead(differentiable): static parameter {self.PARAM_FIELDS[j]!r} is an integer leaf and "
                                 "has no gradient")
        outs = _SimAhead.apply(self, init_state, obs_stepsize, action_stepsize, tuple(j for j, _ in params), actions, *leaves,
                               *[v for _, v in params])
        obs, st_views, last = outs[0], outs[1:1 + S], outs[1 + S:]
        N = st_views[0].shape[1] - 1
        states = self._traj_state(init_state, st_views, (B,), N)
        last_state = self.State(self.PhysicalState(*last), init_state.PRNGKey, self._additions((B,), True), init_state.reference)
        return obs, states, last_state

    # ------------------------------------------------------------------ the explicit form
    def vmap_sim_ahead_vjp(self, states, actions, obs_stepsize, action_stepsize, grad_observations=None, grad_states=None,
                           grad_last_state=None, param_grads=None):
        """Vector-Jacobian product of `vmap_sim_ahead(init_state, actions, obs_stepsize, action_stepsize)`.
        states: the `states` that call returned (its rows are the checkpoints the reverse pass recomputes from);
        grad_observations [B, N+1, obs_dim], grad_states (a State / PhysicalState pytree or a sequence of [B, N+1] leaves, None where
        absent), grad_last_state (likewise, [B] leaves): the cotangents, any of them may be None.
        Returns (grad_actions [B, K, A] — a view of lane-major [K, A, B] memory —, PhysicalState of [B] gradients w.r.t. the
        initial physical state). Derivatives of clamps / clips are 0 on the boundary, of sign 0.
        param_grads: None (default: exactly the 2-tuple above), "per_env" or "sum": a third element, the gradient w.r.t.
        `env_properties.static_params` as an instance of the model's StaticParams — [B] leaves (each environment's own term; the
        properties themselves are broadcast values) or their 0-dim batch sums (fp64 accumulation, the same bits on every run).
        Integer leaves (PMSM's p and deadtime) are None; normalisation bounds are not differentiated. The action and state
        gradients are bit for bit those of the call without param_grads."""
        if param_grads not in (None, "per_env", "sum"):
            raise ValueError(f"vmap_sim_ahead_vjp: param_grads must be None, 'per_env' or 'sum' (got {param_grads!r})")
        why = self._vjp_unsupported()
        if why is not None:
            raise ValueError(f"vmap_sim_ahead_vjp: {why}")
        traj = _leaf_list(states, self.STATE_FIELDS)
        idx = None
        if param_grads is not None:
            idx = [j for j in range(len(self.PARAM_FIELDS)) if _native.lib().excenv_param_differentiable(self.ENV_ID, j) == 1]
        res = self._sim_ahead_vjp_launch(traj, torch.as_tensor(actions), obs_stepsize, action_stepsize, grad_observations,
                                         _leaf_list(grad_states, self.STATE_FIELDS), _leaf_list(grad_last_state, self.STATE_FIELDS),
                                         param_idx=idx)
        if param_grads is None:
            return res[0], self.PhysicalState(*res[1])
        per_env = res[2]
        vals = per_env if param_grads == "per_env" else self._param_grad_sum(per_env)
        by_idx = dict(zip(idx, vals))
        return res[0], self.PhysicalState(*res[1]), self.StaticParams(*[by_idx.get(j) for j in range(len(self.PARAM_FIELDS))])

    def _param_grad_sum(self, per_env):
        """Batch sums of per-environment gradients ([B] tensors of the working dtype): excenv_param_grad_sum -> 0-dim tensors"""
        n, B = len(per_env), self.batch_size
        out = torch.empty(n, dtype=self.dtype, device=self.device)
        ws_bytes = _native.lib().excenv_param_grad_sum_workspace_bytes(_native.dtype_id(self.dtype), B, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        _native._launch("excenv_param_grad_sum", out, "vmap_sim_ahead_vjp(param_grads='sum')", _native.dtype_id(self.dtype), B, n,
                        _native._ptrs(per_env), out.data_ptr(), ws.data_ptr(), ws_bytes)
        return [out[j] for j in range(n)]

    def _lane_major(self, g, shape, strides):
        """g as a tensor of `shape` whose memory is lane-major (`strides`): itself when it is, else a copy."""
        return cotangent(g, self.device, self.dtype, shape, strides)

    def _sim_ahead_vjp_launch(self, traj, actions, obs_stepsize, action_stepsize, g_obs, g_states, g_last, param_idx=None,
                              packed=None):
        """-> (grad_actions, [grad of the initial state leaves]) and, with param_idx (positions in PARAM_FIELDS), a third element:
        the [B] per-environment gradients of those parameters, from the PGRAD launch. packed: the forward's packed properties."""
        B, S, A, OW = self.batch_size, self.physical_state_dim, self.action_dim, self._obs_dim()
        dt, dev = self.dtype, self.device
        assert actions.ndim == 3 and actions.shape[0] == B and actions.shape[2] == A, \
            "The actions need to have three dimensions: (batch_size, n_action_steps, action_dim)"
        K = actions.shape[1]
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        rows = K * sub + 1
        sB = B or 1
        if actions.device != dev or actions.dtype != dt:
            actions = actions.to(device=dev, dtype=dt)
        actions = actions.detach()
        if K > 0 and B > 0 and tuple(actions.stride()) == (1, A * B, B):
            a_layout = _LM
        else:
            actions, a_layout = actions.contiguous(), _EM
        for t in traj:
            if not (isinstance(t, torch.Tensor) and tuple(t.shape) == (B, rows) and (tuple(t.stride()) == (1, sB) or B == 0)
                    and t.dtype is dt and t.is_cuda):
                raise ValueError("vmap_sim_ahead_vjp: `states` must be the lane-major state trajectory a vmap_sim_ahead call with "
                                 "these actions and step sizes returned (the 'env_major' and 'tiled' layouts have no reverse mode)")
        if g_obs is not None:
            g_obs = self._lane_major(g_obs, (B, rows, OW), (1, OW * sB, sB))
        if g_states is not None:
            g_states = [None if g is None else self._lane_major(g, (B, rows), (1, sB)) for g in g_states]
        if g_last is not None:
            g_last = [None if g is None else self._lane_major(g, (B,), (1,)) for g in g_last]
        props, keep = packed if packed is not None else self._props_for(self.env_properties, B)
        control = count_control(self)
        grad_actions = torch.empty((K, A, B), dtype=dt, device=dev)
        grad_in = torch.empty((S, (B + 3) // 4 * 4), dtype=dt, device=dev)  # every leaf 16-byte aligned
        gs = [grad_in[j, :B] for j in range(S)]
        # the transposed copy of row-major actions and, where the saved rows do not determine the steps' starting points (the tank
        # under "ahead" with an RK solver), the raw levels a pass in front of the launch restores
        ws_bytes = _native.lib().excenv_sim_ahead_vjp_workspace_bytes_for(self.ENV_ID, self._solver.id, _native.dtype_id(dt), B, K, sub,
                                                                          self._semantics_id, a_layout)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
        args = (self.ENV_ID, self._solver.id,
                _native.dtype_id(dt), B, K, sub, ctypes.byref(props), _native._ref(control), float(obs_stepsize),
                float(self.tau), actions.data_ptr() if K > 0 else None, a_layout, _native._ptrs(traj), _native._ptr(g_obs),
                opt_ptrs(g_states), opt_ptrs(g_last), grad_actions.data_ptr() if K > 0 else None, _native._ptrs(gs),
                self._semantics_id, _native._ptr(ws), ws_bytes, _native._ref(self.launch_opts))
        if not param_idx:
            _native._launch("excenv_sim_ahead_vjp", grad_actions, "vmap_sim_ahead_vjp", *args)
            self.last_vjp_launch = _native.last_launch()
            return grad_actions.permute(2, 0, 1), gs
        grad_p = torch.empty((len(param_idx), (B + 3) // 4 * 4), dtype=dt, device=dev)  # every leaf 16-byte aligned
        gp = [grad_p[i, :B] for i in range(len(param_idx))]
        slots = [None] * _native.MAX_STATIC
        for i, j in enumerate(param_idx):
            slots[j] = gp[i].data_ptr()
        _native._launch_then("excenv_sim_ahead_vjp_params", grad_actions, "vmap_sim_ahead_vjp", args,
                             ((ctypes.c_void_p * _native.MAX_STATIC)(*slots),))
        self.last_vjp_launch = _native.last_launch()
        return grad_actions.permute(2, 0, 1), gs, gp
