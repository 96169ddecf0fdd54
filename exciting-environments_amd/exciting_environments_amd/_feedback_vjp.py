"""Reverse mode of `vmap_sim_ahead_feedback`: the explicit vector-Jacobian product `vmap_sim_ahead_feedback_vjp` (one
`excenv_sim_feedback_vjp` call, include/excenv.h: the integrator pre-pass, sim_feedback_vjp_kernel, the gain-gradient kernel and the
deterministic batch sum, all enqueued by that one C call) and the `torch.autograd.Function` behind
`vmap_sim_ahead_feedback(..., differentiable=True)`: gradients of a loss on a closed-loop trajectory with respect to the gains, the
feedforward rows, the initial integrator state and the initial physical state. Mixed into `CoreEnvironment`
(core_env.py).

Everything is read lane-major: the tensors `vmap_sim_ahead_feedback` returned are read in place, anything else is copied once.
Gradients with respect to the static parameters, the references, the normalisation bounds and the clip bounds are not computed."""
from __future__ import annotations

import ctypes
import math
from dataclasses import replace

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._reverse import _leaf_list, cotangent, opt_ptrs, unsupported


class _Feedback(torch.autograd.Function):
    """vmap_sim_ahead_feedback with a graph behind its outputs: (gain, integral gain, feedforward, integrator state, initial
    physical-state leaves) -> (observations, state trajectory leaves, last-state leaves, actions[, z]). Forward is the launch the
    method always makes; backward is one call of the explicit form on the saved outputs."""

    @staticmethod
    def forward(ctx, env, init_state, n_actions, steps, clip, gain, integral_gain, feedforward, integrator_state, *leaves):
        ctx.set_materialize_grads(False)
        S = env.physical_state_dim
        det = lambda t: None if t is None else t.detach()
        st = replace(init_state, physical_state=env.PhysicalState(*[t.detach() for t in leaves]))
        ctx.packed = env._props_for(env.env_properties, env.batch_size)  # the values of this forward
        obs, states, last, actions, z = env._feedback_launch(st, det(gain), n_actions, steps[0], steps[1], det(feedforward),
                                                             det(integral_gain), det(integrator_state), clip)
        traj = [getattr(states.physical_state, n) for n in env.STATE_FIELDS]
        lasts = [getattr(last.physical_state, n) for n in env.STATE_FIELDS]
        ctx.env, ctx.init_state, ctx.steps, ctx.clip, ctx.S = env, st, steps, clip, S
        ctx.has = (integral_gain is not None, integrator_state is not None)
        ctx.meta = [None if t is None else (tuple(t.shape), t.device, t.dtype) for t in (gain, integral_gain, feedforward, integrator_state)]
        saved = [det(gain), obs, actions] + traj
        if integral_gain is not None:
            saved.append(det(integral_gain))
        if integrator_state is not None:
            saved.append(det(integrator_state))
        ctx.save_for_backward(*saved)
        return (obs, *traj, *lasts, actions) + ((z,) if z is not None else ())

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obs, *g):
        env, S = ctx.env, ctx.S
        gain, obs, actions, *rest = ctx.saved_tensors
        traj, rest = rest[:S], rest[S:]
        igain = rest.pop(0) if ctx.has[0] else None
        z_in = rest.pop(0) if ctx.has[1] else None
        g_states, g_last, g_act = list(g[:S]), list(g[S:2 * S]), g[2 * S]
        g_z = g[2 * S + 1] if ctx.has[0] else None
        gs, gg, ggi, gff, gz0 = env._feedback_vjp_launch(
            ctx.init_state, gain, obs, traj, actions, ctx.steps[0], ctx.steps[1], igain, z_in, ctx.clip, g_obs,
            g_states if any(t is not None for t in g_states) else None, g_last if any(t is not None for t in g_last) else None,
            g_act, g_z, packed=ctx.packed)
        need = ctx.needs_input_grad

        def like(t, j):  # the gradient in the shape, device and dtype the input had
            if t is None or ctx.meta[j] is None or not need[5 + j]:
                return None
            shape, dev, dt = ctx.meta[j]
            return t.reshape(shape).to(device=dev, dtype=dt)

        return (None,) * 5 + (like(gg, 0), like(ggi, 1), like(gff, 2), like(gz0, 3)) + tuple(
            t if n else None for t, n in zip(gs, need[9:9 + S]))


class FeedbackVjpMixin:
    # excenv_last_launch() of the most recent excenv_sim_feedback_vjp call of this environment, read on the thread that enqueued it
    # (autograd runs backward on a thread of its own), and which cotangent groups that call was handed:
    # {"obs": bool, "states": [bool per leaf], "last_state": [bool per leaf], "actions": bool, "z": bool}
    last_feedback_vjp_launch = ""
    last_feedback_vjp_cotangents = None

    def _feedback_vjp_unsupported(self):
        """The reason this environment's configuration has no reverse mode through the closed loop, or None."""
        if self.traj_layout != "lane_major":
            return (f"traj_layout={self.traj_layout!r}: the closed-loop kernels read and write the 'lane_major' layout only")
        if self.sim_ahead_semantics == "ahead_accumulated_t":
            return ("sim_ahead_semantics='ahead_accumulated_t': a closed loop is a chain of steps ('step' semantics) on every "
                    "setting, and that clock has no reverse mode")
        why = unsupported(self)
        if why is None and self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            why = "graph capture: the reverse call allocates its outputs and workspace"
        return why

    def _feedback_differentiable(self, init_state, gain, n_actions, obs_stepsize, action_stepsize, feedforward, integral_gain,
                                 integrator_state, clip):
        """vmap_sim_ahead_feedback(differentiable=True) with an input that requires grad: records one autograd node."""
        what = "vmap_sim_ahead_feedback(differentiable=True)"
        why = self._feedback_vjp_unsupported()
        if why is None and not self.store_state_trajectory:
            why = "store_state_trajectory=False: the reverse pass reads the state trajectory"
        if why is not None:
            raise ValueError(f"{what}: {why}")
        params = self._param_leaves()
        if params:
            names = ", ".join(repr(self.PARAM_FIELDS[j]) for j, _ in params)
            raise ValueError(f"{what}: static parameter {names} requires grad, and the closed loop has no parameter gradients "
                             "(detach the parameter)")
        B, S = self.batch_size, self.physical_state_dim
        leaves = [torch.as_tensor(getattr(init_state.physical_state, n)) for n in self.STATE_FIELDS]
        opt = lambda t: None if t is None else torch.as_tensor(t)
        outs = _Feedback.apply(self, init_state, n_actions, (obs_stepsize, action_stepsize), clip, torch.as_tensor(gain),
                               opt(integral_gain), opt(feedforward), opt(integrator_state), *leaves)
        obs, traj, last, actions = outs[0], outs[1:1 + S], outs[1 + S:1 + 2 * S], outs[1 + 2 * S]
        z = outs[2 + 2 * S] if integral_gain is not None else None
        N = traj[0].shape[1] - 1
        states = self._traj_state(init_state, traj, (B,), N)
        last_state = self.State(self.PhysicalState(*last), init_state.PRNGKey, self._additions((B,), True), init_state.reference)
        return obs, states, last_state, actions, z

    # ------------------------------------------------------------------ the explicit form
    def vmap_sim_ahead_feedback_vjp(self, init_state, gain, observations, states, actions, obs_stepsize, action_stepsize,
                                    integral_gain=None, integrator_state=None, clip=(-1.0, 1.0), grad_obs=None, grad_states=None,
                                    grad_last_state=None, grad_actions=None, grad_z=None):
        """Vector-Jacobian product of `observations, states, last_state, actions, z = vmap_sim_ahead_feedback(init_state, gain,
        K, obs_stepsize, action_stepsize, feedforward, integral_gain, integrator_state, clip)` -> (g_state0, g_gain,
        g_integral_gain, g_feedforward, g_integrator_state).

        observations, states, actions: what that call returned (read in place; its rows are the checkpoints of the reverse pass).
        init_state gives the references of the controlled fields. grad_obs [B, N+1, OW] (columns of controlled references are
        ignored), grad_states / grad_last_state (State / PhysicalState pytrees or sequences of [B, N+1] / [B] leaves, None where
        absent), grad_actions [B, K, A], grad_z [B, A]: the cotangents of the five outputs, any of them may be None.

        g_state0: PhysicalState of [B] gradients. g_gain / g_integral_gain: shaped like the gains given — [A, OW], summed over the
        batch (fp64 accumulation in a fixed order: the same bits on every run), or [B, A, OW]; the columns of controlled references
        do get gradients. g_feedforward [B, K, A] (present whether or not a feedforward was given: it is the gradient with respect to
        the pre-clamp action). g_integral_gain / g_integrator_state are None where the input was absent.
        A clamp has derivative 0 on and outside its bounds; the other conventions are `vmap_sim_ahead_vjp`'s. Works whatever
        `env.differentiable` says."""
        why = self._feedback_vjp_unsupported()
        if why is not None:
            raise ValueError(f"vmap_sim_ahead_feedback_vjp: {why}")
        if states is None:
            raise ValueError("vmap_sim_ahead_feedback_vjp: `states` is None (store_state_trajectory=False): the reverse pass reads "
                             "the state trajectory")
        traj = _leaf_list(states, self.STATE_FIELDS)
        gs, gg, ggi, gff, gz0 = self._feedback_vjp_launch(
            init_state, gain, observations, traj, actions, obs_stepsize, action_stepsize, integral_gain, integrator_state, clip,
            grad_obs, _leaf_list(grad_states, self.STATE_FIELDS), _leaf_list(grad_last_state, self.STATE_FIELDS), grad_actions, grad_z)
        return self.PhysicalState(*gs), gg, ggi, gff, (gz0 if integrator_state is not None else None)

    def _feedback_vjp_launch(self, init_state, gain, obs, traj, actions, obs_stepsize, action_stepsize, integral_gain, z_in, clip,
                             g_obs, g_states, g_last, g_actions, g_z, packed=None):
        """-> ([grad of the initial state leaves], g_gain, g_integral_gain or None, g_feedforward [B, K, A], g_z0 [B, A] or None):
        one excenv_sim_feedback_vjp call. packed: the forward's packed properties."""
        B, S, A, OW = self.batch_size, self.physical_state_dim, self.action_dim, self._obs_dim()
        dt, dev = self.dtype, self.device
        sB = B or 1
        actions = torch.as_tensor(actions)
        assert actions.ndim == 3 and actions.shape[0] == B and actions.shape[2] == A, \
            "The actions need to have three dimensions: (batch_size, n_action_steps, action_dim)"
        K = actions.shape[1]
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        rows = K * sub + 1
        lo, hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
        assert lo <= hi, f"clip needs to be (low, high) with low <= high, but {clip} is given"
        lane = lambda t, shape, strides: cotangent(torch.as_tensor(t), dev, dt, shape, strides)
        actions = lane(actions, (B, K, A), (1, A * sB, sB))
        obs = lane(obs, (B, rows, OW), (1, OW * sB, sB))
        traj = [lane(t, (B, rows), (1, sB)) for t in traj]
        # one gain_batch for both sets, as the forward: a broadcast set next to a per-environment one is repeated, and its gradient
        # summed over the batch afterwards
        g, Bg = self._lane_major_gain(gain, "The gain")
        gi, Bgi = (None, Bg) if integral_gain is None else self._lane_major_gain(integral_gain, "The integral gain")
        repeat = lambda t: t[:, :, None].expand(A, OW, B).contiguous().permute(2, 0, 1)
        if Bgi != Bg:
            if Bg == 1:
                g = repeat(g)
            else:
                gi = repeat(gi)
        Bc = max(Bg, Bgi)
        if z_in is not None:
            assert gi is not None, "integrator_state without integral_gain"
            z_in = self._t(torch.as_tensor(z_in).detach(), (B, A)).t().contiguous()  # [A][B]
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
        if g_z is not None:
            g_z = lane(g_z, (B, A), (1, sB)) if gi is not None else None
        props, _keep = packed if packed is not None else self._props_for(self.env_properties, B)
        control, _refs = self._control(init_state, (B,))
        new = lambda *shape: torch.empty(shape, dtype=dt, device=dev)
        grad_in = new(S, (B + 3) // 4 * 4)  # every leaf 16-byte aligned
        gs = [grad_in[j, :B] for j in range(S)]
        g_ff = new(K, A, B)
        g_zi = new(K, A, B) if gi is not None else None
        g_z0 = new(A, B) if gi is not None else None
        gg = new(A, OW, Bc)
        ggi = new(A, OW, Bc) if gi is not None else None
        self.last_feedback_vjp_cotangents = {
            "obs": g_obs is not None, "states": [False] * S if g_states is None else [t is not None for t in g_states],
            "last_state": [False] * S if g_last is None else [t is not None for t in g_last], "actions": g_actions is not None,
            "z": g_z is not None}
        if B > 0:  # (an empty batch has no addresses to hand over)
            # the pointer arrays stay alive in these names until the call has returned: the structure holds their addresses only
            p_traj, p_gst, p_glast, p_gs = _native._ptrs(traj), opt_ptrs(g_states), opt_ptrs(g_last), _native._ptrs(gs)
            addr = lambda arr: None if arr is None else ctypes.addressof(arr)
            call = _native.FeedbackVjp(g.data_ptr(), _native._ptr(gi), Bc, lo, hi, obs.data_ptr(), addr(p_traj),
                                       actions.data_ptr() if K > 0 else None, _native._ptr(z_in), _native._ptr(g_obs), addr(p_gst),
                                       addr(p_glast), _native._ptr(g_actions), _native._ptr(g_z), addr(p_gs),
                                       g_ff.data_ptr() if K > 0 else None, g_zi.data_ptr() if (g_zi is not None and K > 0) else None,
                                       _native._ptr(g_z0), gg.data_ptr(), _native._ptr(ggi))
            ws_bytes = _native.lib().excenv_sim_feedback_vjp_workspace_bytes(self.ENV_ID, _native.dtype_id(dt), B, K,
                                                                             len(self.control_state), Bc, int(gi is not None))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
            _native._launch("excenv_sim_feedback_vjp", grad_in, "vmap_sim_ahead_feedback_vjp", self.ENV_ID, self._solver.id,
                            _native.dtype_id(dt), B, K, sub, ctypes.byref(props), _native._ref(control), float(obs_stepsize),
                            float(self.tau), ctypes.byref(call), _native._ptr(ws), ws_bytes, _native._ref(self.launch_opts))
            del p_traj, p_gst, p_glast, p_gs
            self.last_feedback_vjp_launch = _native.last_launch()

        def shaped(t, given):  # [A][OW][Bc] -> the shape of the gain given: [A, OW] (summed where it was repeated) or [B, A, OW]
            if t is None:
                return None
            if torch.as_tensor(given).ndim == 3:
                return t.permute(2, 0, 1)
            return t[:, :, 0] if Bc == 1 else t.permute(2, 0, 1).sum(0)

        return gs, shaped(gg, gain), shaped(ggi, integral_gain), g_ff.permute(2, 0, 1), (g_z0.t() if g_z0 is not None else None)
