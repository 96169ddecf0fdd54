"""Batched linearisation of the discrete-time model: `vmap_linearize` (the Jacobians A_d = d x+ / d x and B_d = d x+ / d a of one
`vmap_step`, or those of its observation) and `vmap_linearize_ahead` (the same for every step of a stored state trajectory), each one
launch of step_jac_kernel through `excenv_step_jacobian` (include/excenv.h). Mixed into `CoreEnvironment` (core_env.py).

The kernel holds a step's two states and its action in registers and writes the Jacobian row by row, every row the arithmetic of
`vmap_step_vjp` for a one-hot cotangent. The output is lane-major ([R, S + A, B], [N, R, S + A, B] for a trajectory): what is
returned are views of that one allocation. Nothing here records a graph: the matrices are plain tensors."""
from __future__ import annotations

import ctypes

import torch

from . import _native
from ._reverse import _leaf_list, unsupported


class LinearizeMixin:
    # excenv_last_launch() of the most recent excenv_step_jacobian launch of this environment
    last_linearize_launch = ""

    def _linearize_unsupported(self):
        """The reason this environment's configuration has no linearisation, or None. Touches no device."""
        return unsupported(self, saturated="the saturated PMSM has no reverse mode, and the Jacobian rows are its products")

    def _jac_rows(self, rows):
        """-> (row kind id, R)"""
        if rows not in _native.JAC_ROWS:
            raise ValueError(f"rows must be 'state' or 'obs' (got {rows!r})")
        return _native.JAC_ROWS[rows], (self.physical_state_dim if rows == "state" else self._obs_dim() - len(self.control_state))

    def vmap_linearize(self, state, action, new_state=None, rows="state"):
        """The linearisation of `obs, new_state = vmap_step(state, action)` per environment -> (A, Bu): A [B, R, S] =
        d row / d state, Bu [B, R, action_dim] = d row / d action, with R = S rows (the leaves of new_state, rows="state") or
        R = O rows (the model's observation columns, rows="obs"; the columns of controlled references are constants and have no
        rows). Columns are ordered as STATE_FIELDS, then the action components. Both are views of one lane-major [R, S + A, B]
        allocation.

        new_state: the state that vmap_step call returned (read, not recomputed); None: the forward launch is made here, under
        `torch.no_grad()`.

        Definition: row r is exactly what `vmap_step_vjp(state, action, new_state, grad_state=e_r)` returns (rows="obs":
        `grad_obs=e_r`), e_r the one-hot cotangent. So derivatives of clamps and clips are 0 on the boundary and of sign 0, wrapped
        angles have slope 1; static parameters, references and normalisation bounds are not differentiated; PMSM's constant
        omega_el and its buffered voltages have their rows and columns.

        Works whatever `env.differentiable` says; inputs are detached and the outputs carry no graph (differentiating a
        linearisation is out of scope)."""
        why = self._linearize_unsupported()
        if why is not None:
            raise ValueError(f"vmap_linearize: {why}")
        kind, R = self._jac_rows(rows)
        B, S, A = self.batch_size, self.physical_state_dim, self.action_dim
        action = torch.as_tensor(action).detach()
        assert tuple(action.shape) == (B, A), (
            "The action needs to be of shape (batch_size, action_dim) which is " + f"{(B, A)}, but {tuple(action.shape)} is given")
        if action.device != self.device or action.dtype != self.dtype:
            action = action.to(device=self.device, dtype=self.dtype)
        st_in = [self._t(l.detach() if isinstance(l, torch.Tensor) else l, (B,)) for l in _leaf_list(state, self.STATE_FIELDS)]
        if new_state is None:
            with torch.no_grad():
                new_state = self._vmap_step_launch(state, action, False)[-1]
        st_out = [self._t(l.detach() if isinstance(l, torch.Tensor) else l, (B,)) for l in _leaf_list(new_state, self.STATE_FIELDS)]
        buf = torch.empty((R, S + A, B), dtype=self.dtype, device=self.device)
        if B > 0:
            self._step_jacobian_launch(buf, 1, 1, float(self.tau), st_in, st_out, 0, action, (0, action.stride(1), action.stride(0)), kind)
        jac = buf.permute(2, 0, 1)
        return jac[:, :, :S], jac[:, :, S:]

    def vmap_linearize_ahead(self, states, actions, obs_stepsize, action_stepsize, rows="state"):
        """The linearisations of every step n -> n + 1 of a stored trajectory, in one launch -> (A, Bu): A [B, N, R, S],
        Bu [B, N, R, action_dim]; `[:, n]` is `vmap_linearize(row n, actions[:, n // substeps], row n + 1, rows)` bit for bit.
        states: the lane-major `states` a `vmap_sim_ahead(init_state, actions, obs_stepsize, action_stepsize)` call returned,
        N + 1 = K * substeps + 1 rows; actions: that call's [B, K, action_dim] (a lane-major view, `new_actions_buffer`, is read in
        place; anything else is made lane-major by one copy).

        Defined for `sim_ahead_semantics == "step"`, where a trajectory is a chain of steps on the saved, post-processed rows;
        under "ahead" and "ahead_accumulated_t" the carried state is not the saved row, and both are refused.

        The output has N * R * (S + A) * B elements (PMSM, rows="state": 63 per step and environment): mind N at large batch
        sizes. Conventions, `rows` and the absence of a graph as in `vmap_linearize`."""
        why = self._linearize_unsupported()
        if why is None and self.sim_ahead_semantics != "step":
            why = (f"sim_ahead_semantics={self.sim_ahead_semantics!r}: the carried state there is not the saved row, a stored "
                   "trajectory is a chain of steps under 'step' only")
        if why is None and self.traj_layout != "lane_major":
            why = f"traj_layout={self.traj_layout!r}: the Jacobian kernel reads the 'lane_major' state trajectory only"
        if why is not None:
            raise ValueError(f"vmap_linearize_ahead: {why}")
        kind, R = self._jac_rows(rows)
        B, S, A = self.batch_size, self.physical_state_dim, self.action_dim
        dt, dev = self.dtype, self.device
        actions = torch.as_tensor(actions).detach()
        assert actions.ndim == 3 and actions.shape[0] == B and actions.shape[2] == A, \
            "The actions need to have three dimensions: (batch_size, n_action_steps, action_dim)"
        K = actions.shape[1]
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        N = K * sub
        sB = B or 1
        traj = [t.detach() if isinstance(t, torch.Tensor) else t for t in _leaf_list(states, self.STATE_FIELDS)]
        for t in traj:
            if not (isinstance(t, torch.Tensor) and tuple(t.shape) == (B, N + 1) and (tuple(t.stride()) == (1, sB) or B == 0)
                    and t.dtype is dt and t.device == dev):
                raise ValueError("vmap_linearize_ahead: `states` must be the lane-major state trajectory a vmap_sim_ahead call with "
                                 "these actions and step sizes returned")
        if actions.device != dev or actions.dtype != dt:
            actions = actions.to(device=dev, dtype=dt)
        if K > 0 and B > 0 and tuple(actions.stride()) != (1, A * B, B):
            lane_major = self.new_actions_buffer(K)
            lane_major.copy_(actions)
            actions = lane_major
        buf = torch.empty((N, R, S + A, B), dtype=dt, device=dev)
        if N > 0 and B > 0:
            self._step_jacobian_launch(buf, N, sub, float(obs_stepsize), traj, [t[:, 1:] for t in traj], B, actions, (A * B, B, 1), kind)
        jac = buf.permute(3, 0, 1, 2)
        return jac[..., :S], jac[..., S:]

    def _step_jacobian_launch(self, buf, rows, sub, dt, st_in, st_out, s_row, action, a_strides, kind):
        """One excenv_step_jacobian launch into buf ([rows][R][S + A][B]). st_in / st_out: the leaves of the first step, later steps
        s_row elements further; a_strides: the action's (row, component, environment) element strides."""
        B = self.batch_size
        props, _keep = self._props_for(self.env_properties, B)
        _native._launch("excenv_step_jacobian", buf, "vmap_linearize", self.ENV_ID, self._solver.id, _native.dtype_id(self.dtype), B,
                        rows, sub, ctypes.byref(props), len(self.control_state), dt, float(self.tau), _native._ptrs(st_in),
                        _native._ptrs(st_out), s_row, action.data_ptr(), a_strides[0], a_strides[1], a_strides[2], kind,
                        buf.data_ptr(), _native._ref(self.launch_opts))
        self.last_linearize_launch = _native.last_launch()
