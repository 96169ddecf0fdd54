"""How a `vmap_sim_ahead` / `sim_ahead` call becomes ONE launch of the trajectory kernel, in three steps:
1. resolve the call (`_run_sim_ahead`, `_route`): the layout of the incoming actions, the trajectory layout, the effective launch
   options, the optional transposition workspace, the gym-output arrays — everything that does not depend on where the outputs live;
2. provide the outputs (`_outputs_*`): the caller's own triple for `out=`, one shared allocation for small calls, the pooled and
   placed sets of `_placement.py` for large ones, one plain allocation per array for the rest;
3. launch: a single ctypes call with plain arguments (`_native.sim_ahead_raw` -> `excenv_sim_ahead_ws`, include/excenv.h).
Mixed into `CoreEnvironment` (core_env.py), which keeps the reference's API surface: argument checks, shapes, pytrees."""
from __future__ import annotations

import ctypes

import torch

from . import _native

_EM, _LM, _TILED = _native.LAYOUT_ENV_MAJOR, _native.LAYOUT_LANE_MAJOR, _native.LAYOUT_TILED
_TRAJ_LAYOUTS = {"lane_major": _LM, "env_major": _EM, "tiled": _TILED}


def _padded(B, rows, OW, isz):
    """Element counts of the lane-major observation block, one state leaf and one last-state leaf, each a multiple of 16 bytes."""
    al = 16 // isz
    m = al - 1
    return (rows * OW * B + m) // al * al, (rows * B + m) // al * al, (B + m) // al * al


def _lane_major_obs(buf, B, rows, OW):
    """[B, rows, OW] observations over the [rows, OW, B] memory at the start of buf."""
    sB = B or 1  # the strides torch gives the views of an empty array
    return buf.as_strided((B, rows, OW), (1, OW * sB, sB))


def _lane_major_leaves(buf, n, B, rows, leaf_e=0, offset=0):
    """n [B, rows] state leaves over [rows, B] memory: leaf j starts at element offset + j * leaf_e of buf."""
    return buf.as_strided((n, B, rows), (leaf_e, 1, B or 1), offset).unbind(0)


class TrajectoryLaunchMixin:
    # Trajectories up to this size come out of ONE allocation (observations, state leaves and last_state are views of it):
    # at RL / MPC batch sizes the launch takes ~100 us and 2 S + 1 allocator calls plus as many view objects cost as much.
    # Larger outputs keep one allocation per returned array so that dropping the states frees their memory.
    _SHARED_TRAJ_BYTES = 32 << 20

    def _run_sim_ahead(self, init_state, actions, env_properties, obs_stepsize, action_stepsize, B, want_gym=False, out=None,
                       packed=None):
        S, A, OW = self.physical_state_dim, self.action_dim, self._obs_dim()
        actions = torch.as_tensor(actions)
        K = actions.shape[-2]
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        N = K * sub
        rows = N + 1
        props, keep = packed if packed is not None else self._props_for(env_properties, B)  # packed: a differentiable call's own
        st_in = [self._t(getattr(init_state.physical_state, n), (B,)) for n in self.STATE_FIELDS]
        control, refs = self._control(init_state, (B,))
        dt, dev = self.dtype, self.device
        isz = 4 if dt is torch.float32 else 8

        if actions.device != dev or actions.dtype != dt:
            actions = actions.to(device=dev, dtype=dt)
        T = _native.TILE
        if actions.ndim == 4:  # [B/T, T, K, A] view over tiled [B/T, K, A, T] memory (new_actions_buffer(layout="tiled"))
            assert tuple(actions.shape[:2]) == (B // T, T) and tuple(actions.stride()) == (K * A * T, 1, A * T, T), \
                "4-D actions must come from new_actions_buffer(K, layout='tiled')"
            a_layout = _TILED
        elif K > 0 and B > 0 and tuple(actions.stride()) == (1, A * B, B):
            a_layout = _LM  # a [K, A, B] buffer viewed as [B, K, A]
        else:
            actions = actions.contiguous()
            a_layout = _EM

        t_layout, want_states, opts, ws_bytes, provider = self._route(
            B, K, sub, a_layout, want_gym, out is not None, B > 0 and dev.type == "cuda", props, actions, st_in)

        gym_out = gym_ref = None
        if want_gym:  # reward / terminated / truncated trajectories from the same launch (excenv_traj_gym_t), in the trajectory layout
            TW = _native.truncated_width(self.ENV_ID, len(self.control_state))
            if t_layout == _LM:  # reward / terminated [N][B], truncated [N + 1][B][TW]
                rew = torch.empty((N, B), dtype=dt, device=dev)
                term = torch.empty((N, B), dtype=torch.bool, device=dev)
                trunc = torch.empty((N + 1, B, TW), dtype=torch.bool, device=dev)
                gym_out = (rew.t()[..., None], trunc.permute(1, 0, 2), term.t()[..., None])
            else:
                rew = torch.empty((B, N, 1), dtype=dt, device=dev)
                term = torch.empty((B, N, 1), dtype=torch.bool, device=dev)
                trunc = torch.empty((B, N + 1, TW), dtype=torch.bool, device=dev)
                gym_out = (rew, trunc, term)
            gym_struct = _native.TrajGym(rew.data_ptr(), term.data_ptr(), trunc.data_ptr())
            gym_ref = ctypes.byref(gym_struct)
        ws_ptr = None
        if ws_bytes and provider != "shared":
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)  # stream-ordered: free to die when this function returns
            ws_ptr = ws.data_ptr()
        sem = self._semantics_id
        st_in_ptrs = _native._ptrs(st_in)

        def launch(o_ptr, t_ptrs, l_ptrs, keep=False):  # the trajectory launch of this call into the given output buffers
            # keep: the buffers still hold an earlier launch's constant columns (only _placement.launch_into says so)
            o = opts if not keep else _native.launch_opts(
                opts.envs_per_lane if opts else 0, opts.env_major_mode if opts else 0, opts.lds_pad_bytes if opts else 0,
                (opts.flags if opts else 0) | _native.OPT_KEEP_CONSTANT_COLUMNS)
            with _native._on_device(dev):
                _native.sim_ahead_raw(self.ENV_ID, self._solver.id, 0 if dt is torch.float32 else 1, B, K, sub, ctypes.byref(props),
                                      _native._ref(control), float(obs_stepsize), float(self.tau), st_in_ptrs,
                                      actions.data_ptr() if K > 0 else None, a_layout, o_ptr, t_ptrs if want_states else None,
                                      t_layout, l_ptrs, sem, ws_ptr, ws_bytes if ws_ptr is not None else 0, _native._ref(o),
                                      _native._raw_stream(dev), gym_ref)

        if provider == "out":
            res = self._outputs_from_caller(out, B, rows, OW, want_states)
        elif provider == "shared":
            res, ws_ptr = self._outputs_shared(B, rows, OW, S, isz, want_states, ws_bytes)
        elif provider == "placed":
            # lane-major sets: the launch's access pattern can be replayed without arithmetic to judge a placement, for lane-major
            # actions and for row-major ones (the replay then reads the same K * A * B values in lane-major order — the actions are
            # 12 % of the traffic at most and what is being judged is where the OUTPUTS lie; without it such calls fell back to
            # timing the launch itself into candidate blocks, and a traced process sat at 6.5 ms where the bench had 5.0)
            pctx = (actions.data_ptr(), A) if (t_layout == _LM and a_layout in (_LM, _EM) and sub == 1 and K >= 9) else None
            ts = self._placement.acquire(B, rows, OW, S, want_states, _padded(B, rows, OW, isz)[2], isz, launch,
                                         env_major=t_layout == _EM, pattern_ctx=pctx)
            res = (ts.observations, ts.st_views, ts.last, ts.obs_ptr, ts.traj_ptrs, ts.last_ptrs, ts)
        else:
            res = self._outputs_plain(t_layout, B, rows, OW, S, want_states)
        observations, st_views, last, obs_ptr, traj_ptrs, last_ptrs, ts = res

        self.last_constant_columns_kept = False
        if ts is None:
            launch(obs_ptr, traj_ptrs, last_ptrs)
        else:
            self._placement.drain_waits()
            self.last_constant_columns_kept = self._placement.launch_into(
                ts, launch, (OW + (S if want_states else 0)) * rows * B * isz, t_layout == _LM, self.keep_constant_columns,
                _native.cuda_is_capturing())
        if want_gym:
            return observations, st_views, last, N, gym_out
        return observations, st_views, last, N

    # ------------------------------------------------------------------ step 1: host decisions (no allocation, no launch)
    def _route(self, B, K, sub, a_layout, want_gym, has_out, on_gpu, props, actions, st_in):
        """-> (trajectory layout id, want_states, effective launch options, workspace bytes (0: none), output provider: "out" /
        "shared" / "placed" / "plain"). on_gpu: B > 0 on a HIP device; actions / st_in are read for their addresses only."""
        if self.traj_layout not in _TRAJ_LAYOUTS:
            raise ValueError(f"traj_layout must be 'lane_major', 'env_major' or 'tiled', got {self.traj_layout!r}")
        t_layout = _TRAJ_LAYOUTS[self.traj_layout]
        lane_fast = t_layout == _LM and on_gpu
        if has_out and (want_gym or not lane_fast):
            raise ValueError("vmap_sim_ahead(out=...) is available for the default lane-major trajectories without gym outputs")
        if t_layout == _TILED:
            # opt-in, NOT reference-shaped: tiles of T envs, each tile lane-major -> views [B/T, T, N+1, OW] / [B/T, T, N+1]
            assert B % _native.TILE == 0, f"traj_layout='tiled' needs batch_size % {_native.TILE} == 0"
            if want_gym:
                raise ValueError("return_rew_trunc_term is not available with traj_layout='tiled'")
        S, OW, dt = self.physical_state_dim, self._obs_dim(), self.dtype
        isz = 4 if dt is torch.float32 else 8
        rows = K * sub + 1
        want_states = self.store_state_trajectory
        n_control = len(self.control_state)
        row_major = _EM in (a_layout, t_layout)

        # env_major_fused = False: never a fused kernel for row-major buffers. env_major_mode = 1 says so for row-major trajectories
        # (sim_plan.hpp fused_env_major), EXCENV_OPT_NO_FUSED_ACTIONS for row-major actions with lane-major trajectories
        # (reads_row_major_actions) — the only plan that reads a flag, so only those calls carry flags: the caller's and that one.
        # Every other overridden call gets flags = 0, as it always has (a caller's flags are dropped there: the one defined flag
        # means nothing for them). That includes lane-major trajectories that launch nothing (B == 0) or fail before the library is
        # reached (a CPU device).
        opts = self.launch_opts
        if row_major and not self.env_major_fused:
            flags = ((opts.flags if opts else 0) | _native.OPT_NO_FUSED_ACTIONS) if lane_fast else 0
            opts = _native.launch_opts(opts.envs_per_lane if opts else 0, 1, opts.lds_pad_bytes if opts else 0, flags)

        # row-major actions (a plain [B, K, A] tensor, what the reference's call hands over) with lane-major trajectories: large
        # batches of broadcast-property environments read them inside the trajectory kernel (per-wave LDS piece ring, DESIGN.md
        # §4.1b) and need no workspace. The launch fuses only when every state array allows 16-byte accesses as well (launch.hpp:
        # vec_ok); the output arrays made here always do. A "fused" answer for a call that then does not fuse would skip the
        # workspace and drop the call to the generic-stride read of the actions — correct, but far slower than the transposition it
        # replaced. (the query describes the step and ahead semantics: accumulated-time calls never fuse, so they always get the
        # workspace)
        fuses = False
        if lane_fast and a_layout == _EM:
            aligned = all(t.data_ptr() % 16 == 0 for t in st_in)
            fk = (B, K, sub, n_control, actions.data_ptr() % 16, id(props), bool(want_gym), aligned,
                  None if opts is None else (opts.envs_per_lane, opts.flags), self._semantics_id)
            if self._fused_actions_cache is None or self._fused_actions_cache[0] != fk:
                self._fused_actions_cache = (fk, aligned and self._semantics_id != _native.SEM_AHEAD_ACCUMULATED_T
                                             and _native.sim_ahead_fuses_actions(self.ENV_ID, self._solver.id, dt, B, K, props, n_control,
                                                                                 bool(want_gym), a_layout, t_layout, actions.data_ptr(), opts))
            fuses = self._fused_actions_cache[1]
        # other row-major buffers: let the library transpose through a scratch buffer instead of issuing scattered 4-byte accesses
        ws_bytes = 0
        if row_major and self.env_major_workspace and B > 0 and not fuses:
            wk = (B, K, sub, n_control, want_states, a_layout, t_layout)
            if self._ws_bytes_cache is None or self._ws_bytes_cache[0] != wk:
                self._ws_bytes_cache = (wk, _native.sim_ahead_workspace_bytes(self.ENV_ID, dt, B, K, sub, n_control, a_layout, t_layout,
                                                                              want_states))
            ws_bytes = self._ws_bytes_cache[1]

        if lane_fast:
            obs_e, leaf_e, last_e = _padded(B, rows, OW, isz)
            total = obs_e + (S * leaf_e if want_states else 0) + S * last_e + (ws_bytes + 15) // 16 * (16 // isz)
            provider = "out" if has_out else "shared" if total * isz <= self._SHARED_TRAJ_BYTES else "placed"
        elif (t_layout == _EM and on_gpu and not want_gym
              and (OW + (S if want_states else 0)) * rows * B * isz >= self._placement.PLACED_BYTES):
            # row-major (reference-shaped) trajectories: the fused env-major kernels write scattered runs and depend on where
            # observations and state leaves lie even more than the lane-major kernel does (tools/em_placement.py: 7.0 ... 10.9 ms
            # for the same launch), so these sets are pooled and placed like the lane-major ones
            provider = "placed"
        else:
            provider = "plain"
        return t_layout, want_states, opts, ws_bytes, provider

    # ------------------------------------------------------------------ step 2: where the outputs live
    # Each provider returns (observations, st_views, last, obs_ptr, traj_ptrs, last_ptrs, TrajSet to time the launch against or None).
    def _outputs_from_caller(self, out, B, rows, OW, want_states):
        """The caller hands back what an earlier call of the same shape returned: same buffers, no allocation."""
        dt, dev = self.dtype, self.device
        observations, o_states, o_last = out
        on_dev = lambda t: t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)
        ok = (isinstance(observations, torch.Tensor) and observations.dtype is dt and on_dev(observations)
              and tuple(observations.shape) == (B, rows, OW) and tuple(observations.stride()) == (1, OW * B, B))
        last = tuple(getattr(o_last.physical_state, n) for n in self.STATE_FIELDS)
        ok = ok and all(isinstance(t, torch.Tensor) and t.dtype is dt and on_dev(t) and tuple(t.shape) == (B,)
                        and t.is_contiguous() for t in last)
        st_views = None
        if want_states:
            ok = ok and o_states is not None
            st_views = tuple(getattr(o_states.physical_state, n) for n in self.STATE_FIELDS) if ok else None
            ok = ok and all(isinstance(t, torch.Tensor) and t.dtype is dt and on_dev(t)
                            and tuple(t.shape) == (B, rows) and tuple(t.stride()) == (1, B) for t in st_views)
        if not ok:
            raise ValueError("vmap_sim_ahead(out=...): pass the (observations, states, last_state) an earlier call with the "
                             "same batch, horizon, layout and dtype returned")
        return observations, st_views, last, observations.data_ptr(), _native._ptrs(st_views), _native._ptrs(last), None

    def _outputs_shared(self, B, rows, OW, S, isz, want_states, ws_bytes):
        """Lane-major buffers carved from one allocation, pointers computed from its base address. The workspace is carved from
        the same buffer, behind them: -> (the providers' record, workspace address or None)."""
        obs_e, leaf_e, last_e = _padded(B, rows, OW, isz)
        traj_e = obs_e + (S * leaf_e if want_states else 0)
        ws_off = traj_e + S * last_e
        buf = torch.empty(ws_off + (ws_bytes + 15) // 16 * (16 // isz), dtype=self.dtype, device=self.device)
        base = buf.data_ptr()
        st_views = traj_ptrs = None
        if want_states:
            st_views = _lane_major_leaves(buf, S, B, rows, leaf_e, obs_e)
            traj_ptrs = _native.ptr_array([base + (obs_e + j * leaf_e) * isz for j in range(S)])
        last = buf.as_strided((S, B), (last_e, 1), traj_e).unbind(0)
        last_ptrs = _native.ptr_array([base + (traj_e + j * last_e) * isz for j in range(S)])
        return ((_lane_major_obs(buf, B, rows, OW), st_views, last, base, traj_ptrs, last_ptrs, None),
                base + ws_off * isz if ws_bytes else None)

    def _outputs_plain(self, t_layout, B, rows, OW, S, want_states):
        """One allocation per returned array (any layout; where nothing can be launched, this is what says so)."""
        T = _native.TILE
        new = lambda *shape: torch.empty(shape, dtype=self.dtype, device=self.device)
        leaves = lambda *shape: [new(*shape) for _ in range(S)] if want_states else None
        if t_layout == _LM:
            obs_buf, st_buf = new(rows, OW, B), leaves(rows, B)
            observations = _lane_major_obs(obs_buf, B, rows, OW)
            st_views = [_lane_major_leaves(b, 1, B, rows)[0] for b in st_buf] if want_states else None
        elif t_layout == _TILED:  # views [B/T, T, rows, OW] / [B/T, T, rows]
            obs_buf, st_buf = new(B // T, rows, OW, T), leaves(B // T, rows, T)
            observations = obs_buf.permute(0, 3, 1, 2)
            st_views = [b.permute(0, 2, 1) for b in st_buf] if want_states else None
        else:
            observations, st_views = obs_buf, st_buf = new(B, rows, OW), leaves(B, rows)
        _native._require_device(obs_buf, "vmap_sim_ahead")
        last = [new(B) for _ in range(S)]
        return observations, st_views, last, obs_buf.data_ptr(), _native._ptrs(st_buf), _native._ptrs(last), None
