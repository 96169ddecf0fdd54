"""Reverse mode of `vmap_sim_ahead_policy`: the explicit vector-Jacobian product `vmap_sim_ahead_policy_vjp` (one
`excenv_sim_policy_vjp` call, include/excenv.h: ONE launch of sim_policy_vjp_kernel, which carries the state cotangent back through the
dynamics and the transposed network and writes the cotangent of the network's pre-clamp output at every action row) and the
`torch.autograd.Function` behind `vmap_sim_ahead_policy(..., differentiable=True)`: gradients of a loss on a policy rollout with
respect to the network's parameters, the noise rows and the initial physical state. Mixed into `CoreEnvironment`
(core_env.py).

The kernel computes no parameter gradient. That one is sum_{b,k} (d mlp / d params)(obs[b, k])^T grad_raw[b, k], a contraction over
B * K independent samples: torch does it here, through `MLPPolicy.torch_forward` on the observation rows the forward saved, in chunks.

Everything is read lane-major: the tensors `vmap_sim_ahead_policy` / `vmap_rollout_episodes` returned are read in place, anything else
is copied once. Gradients with respect to the static parameters, the references, the reset states and the clip bounds are not
computed; there is no second derivative."""
from __future__ import annotations

import ctypes
from dataclasses import replace

import torch
from torch.autograd.function import once_differentiable

from . import _closed_loop, _native
from ._reverse import _leaf_list, cotangent, count_control, opt_ptrs

# samples (environments x action rows) per pass of the parameter contraction: bounds the hidden activations torch materialises
PARAM_CHUNK = 2 ** 21
# `param_grads=` of vmap_sim_ahead_policy_vjp: the torch contraction (True: what it always meant), none, or excenv_policy_param_grad
PARAM_GRAD_ROUTES = (True, "torch", False, "fused")


def _param_grad_route(param_grads):
    """-> "torch", "fused" or None (no parameter gradient)"""
    if param_grads is True or (isinstance(param_grads, str) and param_grads == "torch"):
        return "torch"
    if param_grads is False:
        return None
    if isinstance(param_grads, str) and param_grads == "fused":
        return "fused"
    raise ValueError(f"vmap_sim_ahead_policy_vjp: param_grads needs to be one of True, 'torch', False or 'fused', but {param_grads!r} is given")


class _PolicyRollout(torch.autograd.Function):
    """vmap_sim_ahead_policy with a graph behind its outputs: (policy.params, noise, initial physical-state leaves) ->
    (observations, state trajectory leaves, last-state leaves, actions). Forward is the launch the method always makes; backward is
    one call of the explicit form on the saved outputs."""

    @staticmethod
    def forward(ctx, env, init_state, policy, n_actions, steps, clip, params, noise, *leaves):
        ctx.set_materialize_grads(False)
        S = env.physical_state_dim
        st = replace(init_state, physical_state=env.PhysicalState(*[t.detach() for t in leaves]))
        ctx.packed = env._props_for(env.env_properties, env.batch_size)  # the values of this forward
        obs, states, last, actions = env._policy_launch("vmap_sim_ahead_policy", st, policy, n_actions, steps[0], steps[1],
                                                        None if noise is None else noise.detach(), clip, recording=True)
        traj = [getattr(states.physical_state, n) for n in env.STATE_FIELDS]
        lasts = [getattr(last.physical_state, n) for n in env.STATE_FIELDS]
        ctx.env, ctx.policy, ctx.steps, ctx.clip, ctx.S = env, policy, steps, clip, S
        ctx.meta = [None if t is None else (tuple(t.shape), t.device, t.dtype) for t in (params, noise)]
        ctx.save_for_backward(obs, actions, *traj)
        return (obs, *traj, *lasts, actions)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, *g):
        env, S = ctx.env, ctx.S
        obs, actions, *traj = ctx.saved_tensors
        g_states, g_last, g_act = list(g[:S]), list(g[S:2 * S]), g[2 * S]
        need = ctx.needs_input_grad
        gs, g_noise, g_params = env._policy_vjp_launch(
            ctx.policy, obs, traj, actions, ctx.steps[0], ctx.steps[1], ctx.clip, g_obs,
            g_states if any(t is not None for t in g_states) else None, g_last if any(t is not None for t in g_last) else None,
            g_act, None, env.policy_param_grads if need[6] else False, packed=ctx.packed)

        def like(t, j, wanted):  # the gradient in the shape, device and dtype the input had
            if t is None or ctx.meta[j] is None or not wanted:
                return None
            shape, dev, dt = ctx.meta[j]
            return t.reshape(shape).to(device=dev, dtype=dt)

        return (None,) * 6 + (like(g_params, 0, need[6]), like(g_noise, 1, need[7])) + tuple(
            t if n else None for t, n in zip(gs, need[8:8 + S]))


class PolicyVjpMixin:
    # excenv_last_launch() of the most recent excenv_sim_policy_vjp call of this environment, read on the thread that enqueued it
    # (autograd runs backward on a thread of its own)
    last_policy_vjp_launch = ""
    _policy_param_grads = "torch"

    @property
    def policy_param_grads(self):
        """What `param_grads=True` means in the recording form (`vmap_sim_ahead_policy(differentiable=True)`): "torch", the
        contraction in torch (the default), or "fused", one excenv_policy_param_grad call on the matrix cores."""
        return self._policy_param_grads

    @policy_param_grads.setter
    def policy_param_grads(self, value):
        if not (isinstance(value, str) and value in ("torch", "fused")):
            raise ValueError(f"policy_param_grads needs to be 'torch' or 'fused', but {value!r} is given")
        self._policy_param_grads = value

    def vmap_policy_param_grads(self, policy, observations, grad_raw, obs_stepsize, action_stepsize, max_groups=0):
        """The parameter gradient of a policy rollout on its own: sum over the batch and the action rows of (d mlp / d params)(obs
        row)^T grad_raw row, flat like `policy.params` (in the environment's dtype on its device). One excenv_policy_param_grad call
        (include/excenv.h): policy_param_grad_kernel on the matrix cores and a deterministic fp64 sum, no torch contraction.

        observations [B, N+1, OW]: what `vmap_sim_ahead_policy` / `vmap_rollout_episodes` returned; the rows of the action rows are
        read. grad_raw [B, K, A]: the `g_noise` of `vmap_sim_ahead_policy_vjp` (it already carries an episode mask). Lane-major views
        are read in place, anything else is copied once. max_groups: 0 (auto), or at most this many workgroups — the grouping, and
        with it the bits, are a function of (B, K, max_groups) only."""
        from ._policy import MLPPolicy

        assert isinstance(policy, MLPPolicy), f"policy needs to be an MLPPolicy, but {type(policy).__name__} is given"
        if not (isinstance(max_groups, int) and max_groups >= 0):
            raise ValueError(f"vmap_policy_param_grads: max_groups needs to be a non-negative integer (0: auto), but {max_groups!r} is given")
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        OW, A = policy.widths[0], policy.widths[-1]
        grad_raw = torch.as_tensor(grad_raw)
        if not (grad_raw.ndim == 3 and grad_raw.shape[0] == B and grad_raw.shape[2] == A):
            raise ValueError(f"vmap_policy_param_grads: grad_raw needs to be of shape (batch_size, n_actions, {A}), but "
                             f"{tuple(grad_raw.shape)} is given")
        K = grad_raw.shape[1]
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        rows = K * sub + 1
        observations = torch.as_tensor(observations)
        if tuple(observations.shape) != (B, rows, OW):
            raise ValueError(f"vmap_policy_param_grads: observations need to be of shape {(B, rows, OW)}, but "
                             f"{tuple(observations.shape)} is given")
        obs = cotangent(observations, dev, dt, (B, rows, OW), (1, OW * sB, sB))
        g_raw = cotangent(grad_raw, dev, dt, (B, K, A), (1, A * sB, sB))
        return self._policy_param_grad_launch(policy, policy.on(dev, dt).detach(), obs, g_raw, K, sub, max_groups)

    def _policy_param_grad_launch(self, policy, params, obs, g_raw, K, sub, max_groups):
        """One excenv_policy_param_grad call on lane-major obs ([N+1][OW][B] in memory) and g_raw ([K][A][B] in memory) -> flat
        gradient like `params`. The workspace comes from a cache of this environment, keyed by its byte count."""
        B, dt = self.batch_size, self.dtype
        if B == 0:
            return torch.zeros_like(params)
        out = torch.empty_like(params)
        widths = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*policy.widths)
        record = _native.Policy(params.data_ptr(), policy.n_layers, _native.ACTIVATIONS[policy.activation], widths, None, 0.0, 0.0)
        need = _native.lib().excenv_policy_param_grad_workspace_bytes(_native.dtype_id(dt), B, K, ctypes.byref(record), max_groups)
        if need < 0:
            raise ValueError(f"vmap_policy_param_grads: no workspace size for widths {policy.widths} and max_groups {max_groups}")
        cache = self.__dict__.setdefault("_policy_param_grad_workspaces", {})
        ws = cache.get(need)
        if ws is None or ws.device != params.device:
            ws = cache[need] = torch.empty(max(need // 8, 1), dtype=torch.float64, device=params.device)
        call = _native.PolicyParamGrad(record, obs.data_ptr(), g_raw.data_ptr() if K > 0 else None, out.data_ptr(), ws.data_ptr(),
                                       ws.numel() * 8, max_groups)
        _native._launch("excenv_policy_param_grad", out, "vmap_policy_param_grads", _native.dtype_id(dt), B, K, sub, ctypes.byref(call))
        return out

    def _policy_differentiable(self, init_state, policy, n_actions, obs_stepsize, action_stepsize, noise, clip):
        """vmap_sim_ahead_policy(differentiable=True) with an input that requires grad: records one autograd node."""
        what = "vmap_sim_ahead_policy(differentiable=True)"
        why = self._feedback_vjp_unsupported()
        if why is None and not self.store_state_trajectory:
            why = "store_state_trajectory=False: the reverse pass reads the state trajectory"
        if why is not None:
            raise ValueError(f"{what}: {why}")
        params = self._param_leaves()
        if params:
            names = ", ".join(repr(self.PARAM_FIELDS[j]) for j, _ in params)
            raise ValueError(f"{what}: static parameter {names} requires grad, and the policy rollout has no parameter gradients "
                             "(detach the parameter)")
        B, S = self.batch_size, self.physical_state_dim
        leaves = [torch.as_tensor(getattr(init_state.physical_state, n)) for n in self.STATE_FIELDS]
        outs = _PolicyRollout.apply(self, init_state, policy, n_actions, (obs_stepsize, action_stepsize), clip, policy.params,
                                    None if noise is None else torch.as_tensor(noise), *leaves)
        obs, traj, last, actions = outs[0], outs[1:1 + S], outs[1 + S:1 + 2 * S], outs[1 + 2 * S]
        N = traj[0].shape[1] - 1
        states = self._traj_state(init_state, traj, (B,), N)
        last_state = self.State(self.PhysicalState(*last), init_state.PRNGKey, self._additions((B,), True), init_state.reference)
        return obs, states, last_state, actions

    # ------------------------------------------------------------------ the explicit form
    def vmap_sim_ahead_policy_vjp(self, policy, observations, states, actions, obs_stepsize, action_stepsize, clip=(-1.0, 1.0),
                                  grad_obs=None, grad_states=None, grad_last_state=None, grad_actions=None, reset=None,
                                  param_grads=True):
        """Vector-Jacobian product of `observations, states, last_state, actions = vmap_sim_ahead_policy(init_state, policy, K,
        obs_stepsize, action_stepsize, noise, clip)` -> (g_state0, g_noise, g_params).

        observations, states, actions: what that call returned (read in place; its rows are the checkpoints of the reverse pass, and
        the stored observation rows carry the references of the controlled fields). grad_obs [B, N+1, OW] (columns of controlled
        references are ignored), grad_states / grad_last_state (State / PhysicalState pytrees or sequences of [B, N+1] / [B] leaves,
        None where absent), grad_actions [B, K, A]: the cotangents of the four outputs, any of them may be None.

        g_state0: PhysicalState of [B] gradients. g_noise [B, K, A]: the gradient with respect to the network's pre-clamp output,
        which is the noise's gradient whether or not a noise was given. g_params: flat like `policy.params` (in the environment's
        dtype on its device), summed over the batch and the action rows — `torch.autograd.grad(policy.torch_forward(rows), params,
        g_noise)` over the observation rows of the action rows, accumulated in chunks of at most 2^21 samples; None with
        `param_grads=False` (the launch alone). `param_grads="torch"` is `True`; `param_grads="fused"` computes g_params with one
        excenv_policy_param_grad call instead (`vmap_policy_param_grads`: the matrix cores, a deterministic fp64 sum; g_state0 and
        g_noise keep their bits). Any other value raises a ValueError. The weights on reference columns do get gradients.

        reset [B, K] bool: the episode mask `vmap_rollout_episodes` returned (one solver step per action). Where reset[:, n] is set,
        step n -> n + 1 was a reset: nothing flows from row n + 1 back to row n, reset states get no gradient, and the action of row
        n (written, not applied) receives grad_actions[:, n] only. This is the route to gradients through `vmap_rollout_episodes`.
        A clamp has derivative 0 on and outside its bounds, ReLU has derivative 0 at 0; the other conventions are
        `vmap_sim_ahead_vjp`'s. Works whatever `env.differentiable` says."""
        from ._policy import MLPPolicy

        assert isinstance(policy, MLPPolicy), f"policy needs to be an MLPPolicy, but {type(policy).__name__} is given"
        _param_grad_route(param_grads)  # (refused by name before anything else)
        why = self._feedback_vjp_unsupported()
        if why is not None:
            raise ValueError(f"vmap_sim_ahead_policy_vjp: {why}")
        if states is None:
            raise ValueError("vmap_sim_ahead_policy_vjp: `states` is None (store_state_trajectory=False): the reverse pass reads "
                             "the state trajectory")
        traj = _leaf_list(states, self.STATE_FIELDS)
        gs, g_noise, g_params = self._policy_vjp_launch(
            policy, observations, traj, actions, obs_stepsize, action_stepsize, clip, grad_obs,
            _leaf_list(grad_states, self.STATE_FIELDS), _leaf_list(grad_last_state, self.STATE_FIELDS), grad_actions, reset, param_grads)
        return self.PhysicalState(*gs), g_noise, g_params

    def _policy_vjp_launch(self, policy, obs, traj, actions, obs_stepsize, action_stepsize, clip, g_obs, g_states, g_last, g_actions,
                           reset, param_grads, packed=None):
        """-> ([grad of the initial state leaves], g_noise [B, K, A], g_params flat or None): one excenv_sim_policy_vjp call and the
        parameter contraction, in torch or in one excenv_policy_param_grad call (`param_grads`: PARAM_GRAD_ROUTES). packed: the
        forward's packed properties."""
        route = _param_grad_route(param_grads)
        B, S, A, OW = self.batch_size, self.physical_state_dim, self.action_dim, self._obs_dim()
        dt, dev = self.dtype, self.device
        sB = B or 1
        assert policy.widths[0] == OW and policy.widths[-1] == A, (
            f"The policy needs to map the observation width {OW} to the action width {A}, but its widths are {policy.widths}")
        actions = torch.as_tensor(actions)
        assert actions.ndim == 3 and actions.shape[0] == B and actions.shape[2] == A, \
            "The actions need to have three dimensions: (batch_size, n_action_steps, action_dim)"
        K = actions.shape[1]
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        rows = K * sub + 1
        lo, hi = _closed_loop.clip_bounds(clip)
        lane = lambda t, shape, strides: cotangent(torch.as_tensor(t), dev, dt, shape, strides)
        actions = lane(actions, (B, K, A), (1, A * sB, sB))
        obs = lane(obs, (B, rows, OW), (1, OW * sB, sB))
        traj = [lane(t, (B, rows), (1, sB)) for t in traj]
        if reset is not None:
            assert sub == 1, "reset needs obs_stepsize == action_stepsize (one solver step per action, as vmap_rollout_episodes)"
            reset = torch.as_tensor(reset).detach().to(device=dev, dtype=torch.bool)
            assert tuple(reset.shape) == (B, K), f"reset needs to be of shape (batch_size, n_actions) which is {(B, K)}, but {tuple(reset.shape)} is given"
            if tuple(reset.stride()) != (1, sB):
                reset = reset.t().contiguous().t()  # [K][B] bytes
            reset = reset if K > 0 else None
        if g_obs is not None:
            g_obs = lane(g_obs, (B, rows, OW), (1, OW * sB, sB))
        if g_states is not None:
            g_states = [None if t is None else lane(t, (B, rows), (1, sB)) for t in g_states]
            g_states = g_states if any(t is not None for t in g_states) else None
        if g_last is not None:
            g_last = [None if t is None else lane(t, (B,), (1,)) for t in g_last]
            g_last = g_last if any(t is not None for t in g_last) else None
        if g_actions is not None:
            g_actions = lane(g_actions, (B, K, A), (1, A * sB, sB)) if K > 0 else None
        props, _keep = packed if packed is not None else self._props_for(self.env_properties, B)
        control = count_control(self)
        params = policy.on(dev, dt).detach()
        new = lambda *shape: torch.empty(shape, dtype=dt, device=dev)
        grad_in = new(S, (B + 3) // 4 * 4)  # every leaf 16-byte aligned
        gs = [grad_in[j, :B] for j in range(S)]
        g_raw = new(K, A, B)
        if B > 0:  # (an empty batch has no addresses to hand over)
            # the pointer arrays stay alive in these names until the call has returned: the structure holds their addresses only
            p_traj, p_gst, p_glast, p_gs = _native._ptrs(traj), opt_ptrs(g_states), opt_ptrs(g_last), _native._ptrs(gs)
            addr = lambda arr: None if arr is None else ctypes.addressof(arr)
            widths = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*policy.widths)
            record = _native.Policy(params.data_ptr(), policy.n_layers, _native.ACTIVATIONS[policy.activation], widths, None, lo, hi)
            call = _native.PolicyVjp(record, obs.data_ptr(), addr(p_traj), actions.data_ptr() if K > 0 else None, _native._ptr(reset),
                                     _native._ptr(g_obs), addr(p_gst), addr(p_glast), _native._ptr(g_actions), addr(p_gs),
                                     g_raw.data_ptr() if K > 0 else None)
            _native._launch("excenv_sim_policy_vjp", grad_in, "vmap_sim_ahead_policy_vjp", self.ENV_ID, self._solver.id,
                            _native.dtype_id(dt), B, K, sub, ctypes.byref(props), _native._ref(control), float(obs_stepsize),
                            float(self.tau), ctypes.byref(call), _native._ref(self.launch_opts))
            del p_traj, p_gst, p_glast, p_gs
            self.last_policy_vjp_launch = _native.last_launch()
        g_noise = g_raw.permute(2, 0, 1)
        g_params = None
        if route == "fused":
            g_params = self._policy_param_grad_launch(policy, params, obs, g_raw, K, sub, 0)
        elif route == "torch":
            g_params = torch.zeros_like(params)
            if B > 0 and K > 0:
                rows_k = obs[:, 0:K * sub:sub, :]  # [B, K, OW]: the observation rows of the action rows
                bc = min(B, PARAM_CHUNK)
                kc = max(1, PARAM_CHUNK // bc)
                with torch.enable_grad():
                    p = params.clone().requires_grad_()
                    for b0 in range(0, B, bc):
                        for k0 in range(0, K, kc):
                            x = rows_k[b0:b0 + bc, k0:k0 + kc].reshape(-1, OW)
                            g = g_noise[b0:b0 + bc, k0:k0 + kc].reshape(-1, A)
                            g_params += torch.autograd.grad(policy.torch_forward(x, p), p, g)[0]
        return gs, g_noise, g_params
