"""Batched LQR synthesis on stored linearisations. Mixed into `CoreEnvironment` (core_env.py), next to `LinearizeMixin`.

`vmap_lqr` is ONE `excenv_lqr_backward` call (include/excenv.h: riccati_kernel): the Riccati recursion of finite-horizon LQR, which is
also the backward pass of iLQR, per environment over the Jacobians `vmap_linearize_ahead` wrote (read in place) or over one
`vmap_linearize` pair iterated `n_iter` times (the stationary gain). `lqr_feedback` turns a state-feedback gain into the observation
gain and feedforward `vmap_sim_ahead_feedback` takes, for the models whose observation is the affine normalisation of the state.

The kernel needs no model: the matrices are the caller's. Inputs are read as values and the results carry no graph."""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from . import _native
from ._rollout_stats import _lane_rows

LQRSolution = namedtuple("LQRSolution", ["gain", "feedforward", "value_hessian", "value_gradient", "expected_change", "n_bad"])
LQRSolution.__doc__ = """What `vmap_lqr` returns, views of lane-major allocations in the environment's dtype: `gain` [B, N, A, S] and
`feedforward` [B, N, A] (u_n = feedforward_n + gain_n x_n; N = 1 in the stationary use), `value_hessian` [B, S, S] and `value_gradient`
[B, S] (P and p at row 0: the cost to go is x^T P x / 2 + p . x + const), `expected_change` [B, 2] (sum_n k . Qu and 1/2 sum_n k . Quu k,
the two numbers of an iLQR line search) and `n_bad` [B] int32 (the steps whose Quu + reg I was not positive definite: their gain is 0)."""


def _cost_matrix(m, name, fn, n, dtype, device):
    """A cost matrix -> [n, n] contiguous in the working dtype on the device. Symmetry is checked where the data is on the host already
    (a device tensor is taken as it is: the check would synchronise)."""
    t = torch.as_tensor(m).detach()
    if tuple(t.shape) != (n, n):
        raise ValueError(f"{fn}: {name} needs to be of shape {(n, n)}, but {tuple(t.shape)} is given")
    if t.device.type == "cpu" and not torch.equal(t, t.t()):
        raise ValueError(f"{fn}: {name} needs to be symmetric")
    return t.to(device=device, dtype=dtype).contiguous()


class LqrMixin:
    # excenv_last_launch() of the most recent excenv_lqr_backward launch of this environment
    last_lqr_launch = ""
    # whether the most recent vmap_lqr call read the caller's Jacobian buffer in place (False: it made the one copy)
    last_lqr_in_place = False

    def vmap_lqr(self, A, Bu, Q, R, Qf=None, q=None, r=None, reg=0.0, n_iter=None):
        """The LQR backward pass of all batch_size environments in one kernel launch -> `LQRSolution(gain, feedforward,
        value_hessian, value_gradient, expected_change, n_bad)`: per environment, for the cost
            sum_{n < N} (x_n^T Q x_n / 2 + q_n . x_n + u_n^T R u_n / 2 + r_n . u_n) + x_N^T Qf x_N / 2 + q_N . x_N
        under x_{n+1} = A_n x_n + Bu_n u_n, the gains of u_n = feedforward_n + gain_n x_n from the Riccati recursion in include/excenv.h
        (excenv_lqr_backward; with q and r the derivatives of a cost along a trajectory and x, u the deviations from it, this is the
        backward pass of iLQR, and `expected_change` are the two numbers of its line search).

        Time-varying use: A [B, N, S, S] and Bu [B, N, S, action_dim]. The two views `vmap_linearize_ahead(rows="state")` returned
        are read in place; anything else is copied once into a lane-major buffer. gain is [B, N, A, S].
        Stationary use: A [B, S, S] and Bu [B, S, action_dim] (what `vmap_linearize` returns) with n_iter = N: the same pair for
        every one of N rows, and only row 0 is kept: gain is [B, 1, A, S], the stationary gain once N is large enough.

        Q, Qf [S, S] and R [A, A] are shared by every environment and row (numbers, arrays or tensors; Qf None: Q). They are taken as
        symmetric; that is checked only where they arrive as host data. q [B, N + 1, S] and r [B, N, A]: the linear cost terms, None:
        zeros. reg >= 0 is added to the diagonal of Quu for the solve only (iLQR's regularisation). A step whose Quu + reg I is not
        positive definite (a NaN included) gets gain 0 and feedforward 0 and is counted in `n_bad`.

        Works for every environment whose (S, action_dim) is one of (1, 1), (2, 1), (4, 1), (7, 2): the six models; the saturated
        PMSM included, because the matrices are the caller's. The same call gives the same bits on every run."""
        fn = "vmap_lqr"
        B, S, Na = self.batch_size, self.physical_state_dim, self.action_dim
        dt, dev = self.dtype, self.device
        sB = B or 1
        if (S, Na) not in _native.LQR_SHAPES:
            raise ValueError(f"{fn}: no kernel for n_state={S}, n_action={Na}: the shapes are {_native.LQR_SHAPES}")
        if not (isinstance(reg, (int, float)) and not isinstance(reg, bool) and reg >= 0):  # a NaN fails the comparison
            raise ValueError(f"{fn}: reg needs to be a non-negative number, but {reg!r} is given")
        A, Bu = torch.as_tensor(A).detach(), torch.as_tensor(Bu).detach()
        C = S + Na
        if A.ndim == 3:
            if not (isinstance(n_iter, int) and not isinstance(n_iter, bool) and n_iter >= 0):
                raise ValueError(f"{fn}: A of shape (batch_size, n_state, n_state) is the stationary use, which needs n_iter as a "
                                 f"non-negative integer, but {n_iter!r} is given")
            if tuple(A.shape) != (B, S, S) or tuple(Bu.shape) != (B, S, Na):
                raise ValueError(f"{fn}: A and Bu need to be of shape {(B, S, S)} and {(B, S, Na)}, but {tuple(A.shape)} and "
                                 f"{tuple(Bu.shape)} are given")
            N, rows, store_all, stride = n_iter, min(n_iter, 1), 0, 0
            a_strides, b_strides = (1, C * sB, sB), (1, C * sB, sB)
            buf_shape = (S, C, B)
        else:
            if n_iter is not None:
                raise ValueError(f"{fn}: n_iter goes with A of shape (batch_size, n_state, n_state) only")
            if not (A.ndim == 4 and Bu.ndim == 4 and tuple(A.shape) == (B, A.shape[1], S, S) and tuple(Bu.shape) == (B, A.shape[1], S, Na)):
                raise ValueError(f"{fn}: A and Bu need to be of shape (batch_size, N, n_state, n_state) and (batch_size, N, n_state, "
                                 f"action_dim) with batch_size {B}, n_state {S} and action_dim {Na}, but {tuple(A.shape)} and "
                                 f"{tuple(Bu.shape)} are given")
            N = rows = A.shape[1]
            store_all, stride = 1, S * C * B
            a_strides, b_strides = (1, S * C * sB, C * sB, sB), (1, S * C * sB, C * sB, sB)
            buf_shape = (N, S, C, B)
        # the views of one [.., S, S + A, B] allocation are read in place; anything else is copied once into such a buffer
        elem = A.element_size()
        in_place = (A.device == dev and Bu.device == dev and A.dtype == dt and Bu.dtype == dt and tuple(A.stride()) == a_strides
                    and tuple(Bu.stride()) == b_strides and Bu.data_ptr() == A.data_ptr() + S * sB * elem)
        self.last_lqr_in_place = bool(in_place)
        jac = None  # B == 0 or N == 0: nothing is read
        if B > 0 and N > 0:
            jac = A
            if not in_place:
                jac = torch.empty(buf_shape, dtype=dt, device=dev)
                view = jac.permute(2, 0, 1) if A.ndim == 3 else jac.permute(3, 0, 1, 2)
                view[..., :S].copy_(A)
                view[..., S:].copy_(Bu)
        Qm = _cost_matrix(Q, "Q", fn, S, dt, dev)
        Rm = _cost_matrix(R, "R", fn, Na, dt, dev)
        Qfm = None if Qf is None else _cost_matrix(Qf, "Qf", fn, S, dt, dev)
        qt = None if q is None else _lane_rows(q, "q", fn, dev, dt, (B, N + 1, S), (1, S * sB, sB))
        rt = None if r is None else _lane_rows(r, "r", fn, dev, dt, (B, N, Na), (1, Na * sB, sB))
        gain = torch.empty((rows, Na, S, B), dtype=dt, device=dev)
        ff = torch.empty((rows, Na, B), dtype=dt, device=dev)
        P0 = torch.empty((S, S, B), dtype=dt, device=dev)
        p0 = torch.empty((S, B), dtype=dt, device=dev)
        dV = torch.empty((2, B), dtype=dt, device=dev)
        n_bad = torch.empty((B,), dtype=torch.int32, device=dev)
        if B > 0:
            # (a call without rows reads no Jacobian and writes no gain: both pointers only have to be there)
            call = _native.Lqr(S, Na, (P0 if jac is None else jac).data_ptr(), stride, Qm.data_ptr(), _native._ptr(Qfm), Rm.data_ptr(), _native._ptr(qt),
                               _native._ptr(rt), float(reg), store_all, gain.data_ptr() or P0.data_ptr(), ff.data_ptr(), P0.data_ptr(), p0.data_ptr(),
                               dV.data_ptr(), n_bad.data_ptr())
            _native._launch("excenv_lqr_backward", P0, fn, _native.dtype_id(dt), B, N, ctypes.byref(call))
            self.last_lqr_launch = _native.last_launch()
        return LQRSolution(gain.permute(3, 0, 1, 2), ff.permute(2, 0, 1), P0.permute(2, 0, 1), p0.t(), dV.t(), n_bad)

    def lqr_feedback(self, K, x_ref, u_ref):
        """A state-feedback law u = u_ref + K (x - x_ref) as the observation feedback of `vmap_sim_ahead_feedback` -> (gain
        [B, A, OW], feedforward [B, A]) such that feedforward + gain @ obs_row == u_ref + K (x - x_ref) for the observation row of
        the physical state x.

        K [B, A, S] or [A, S] (e.g. `vmap_lqr(...).gain[:, 0]`): the gain on the physical state in STATE_FIELDS order, in normalised
        action per physical unit, which is what a gain computed from `vmap_linearize`'s matrices is. x_ref [B, S] or [S]: the
        physical state the law regulates to; u_ref [B, A] or [A]: the normalised action that holds it.

        For the models whose observation is the per-field affine normalisation of the state (pendulum, mass-spring-damper,
        cart-pole, acrobot, fluid tank): obs_j = 2 (x_j - lo_j) / (hi_j - lo_j) - 1, so with h_j = (hi_j - lo_j) / 2
            gain[a, j] = K[a, j] h_j;   feedforward[a] = u_ref[a] + sum_j K[a, j] ((lo_j + h_j) - x_ref[j])
        computed from the environment's normalisation bounds with small torch ops. The columns of controlled references get zero
        gain. The PMSM is refused: its observation holds cos and sin of the angle and is no affine map of the state.

        `vmap_sim_ahead_feedback` takes a feedforward per action row: expand this one with `feedforward[:, None, :].expand(B, K, A)`.
        Angle wrapping is not handled: the observation of a wrapped angle jumps where the state does not, so this is for regulation
        near x_ref, away from the wrap."""
        fn = "lqr_feedback"
        if self.ENV_ID == 5:
            raise ValueError(f"{fn}: the PMSM's observation (cos and sin of the angle, a reordered state) is not an affine map of its "
                             "state: there is no observation gain that equals a state feedback")
        B, S, Na, OW = self.batch_size, self.physical_state_dim, self.action_dim, self._obs_dim()
        dt, dev = self.dtype, self.device

        def arg(t, name, shape):
            t = torch.as_tensor(t).detach().to(device=dev, dtype=dt)
            if tuple(t.shape) not in (shape, (B,) + shape):
                raise ValueError(f"{fn}: {name} needs to be of shape {shape} or {(B,) + shape}, but {tuple(t.shape)} is given")
            return t.expand((B,) + shape)

        K, x_ref, u_ref = arg(K, "K", (Na, S)), arg(x_ref, "x_ref", (S,)), arg(u_ref, "u_ref", (Na,))
        pn = self.env_properties.physical_normalizations

        def bound(v):  # a number or a [B] tensor -> [B] in the working dtype
            v = self._norm_leaf(v)
            return v.expand(B) if isinstance(v, torch.Tensor) else torch.full((B,), v, dtype=dt, device=dev)

        lo = torch.stack([bound(getattr(pn, n).min) for n in self.STATE_FIELDS], dim=-1)   # [B, S]
        hi = torch.stack([bound(getattr(pn, n).max) for n in self.STATE_FIELDS], dim=-1)
        half = (hi - lo) / 2
        gain = torch.zeros((B, Na, OW), dtype=dt, device=dev)
        gain[:, :, :S] = K * half[:, None, :]
        feedforward = u_ref + (K * ((lo + half) - x_ref)[:, None, :]).sum(dim=-1)
        return gain, feedforward
