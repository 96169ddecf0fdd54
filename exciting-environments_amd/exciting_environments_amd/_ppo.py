"""The clipped PPO objective of a diagonal Gaussian policy on the rows a rollout stored. Mixed into
`CoreEnvironment` (core_env.py), next to `PolicyEvalMixin`.

`vmap_gaussian_logp` is the collection-time pass: the log-probabilities of the pre-clamp actions in ONE `excenv_gaussian_logp` call
(include/excenv.h: gaussian_logp_kernel). `vmap_ppo_loss` is the update: ONE `excenv_ppo_loss` call (ppo_loss_kernel and its
reduction) gives a handful of fp64 sums from which the loss and its diagnostics are composed with scalar torch ops, and records one
autograd node whose backward is ONE `excenv_ppo_loss_grad` call (ppo_loss_grad_kernel) that writes the gradient of the means in the
[K][A][B] layout `vmap_policy_eval`'s backward reads in place. With them a PPO epoch on stored rows is
`vmap_policy_eval` -> `vmap_ppo_loss` -> `.backward()`: no elementwise torch pass over the batch and no temporary of its size.

Everything is read lane-major: the views the rollouts, `vmap_policy_eval` and `vmap_gae` returned are read in place, anything else
is copied once. Outputs are plain allocations. Nothing here synchronises with the host."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._policy_eval import _lane_flags
from ._reverse import cotangent

PpoLoss = namedtuple("PpoLoss", ["loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "n"])
PpoLoss.__doc__ = """What `vmap_ppo_loss` returns: 0-dim float64 tensors on the environment's device. `loss` = policy_loss + vf_coef *
value_loss - ent_coef * entropy carries the autograd node; the others carry none. `n` is the number of valid (not `reset`) samples."""

_LOG_2PI = math.log(2.0 * math.pi)


def _scalar(v, device):
    """A number or 0-dim tensor -> 0-dim float64 tensor on the device, without a host synchronisation"""
    if isinstance(v, torch.Tensor):
        return v.detach().to(device=device, dtype=torch.float64).reshape(())
    return torch.full((), float(v), dtype=torch.float64, device=device)


def _number(v, name, fn, lo=None, hi=None):
    if not (isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)) or (lo is not None and not lo < v < hi):
        rng = "a finite number" if lo is None else f"a number in ({lo:g}, {hi:g})"
        raise ValueError(f"{fn}: {name} needs to be {rng}, but {v!r} is given")
    return float(v)


class _PpoObjective(torch.autograd.Function):
    """vmap_ppo_loss with a graph behind `loss`: (mean, value, log_std) -> loss. Forward is the launch the method always makes; backward
    is one excenv_ppo_loss_grad call on the same rows."""

    @staticmethod
    def forward(ctx, env, rows, coef, mean, value, log_std):
        fields = env._ppo_loss_fields(rows, coef)
        ctx.env, ctx.rows, ctx.coef = env, rows, coef
        ctx.metas = [None if t is None else (tuple(t.shape), t.device, t.dtype) for t in (mean, value, log_std)]
        ctx.mark_non_differentiable(*fields[1:])
        return fields

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        env, rows, (vf_coef, ent_coef) = ctx.env, ctx.rows, ctx.coef
        stats = rows["stats"]
        need_mean, need_value, need_std = ctx.needs_input_grad[3:6]
        B, K, A = rows["shape"]
        g = g.detach().to(device=env.device, dtype=torch.float64).reshape(())
        n1 = stats[0].clamp(min=1.0)
        grad_mean = grad_value = grad_std = None
        if need_mean or need_value:
            scale = torch.stack((g / n1, g * vf_coef / n1)).to(env.dtype)
            grad_mean, grad_value = env._ppo_loss_grad_launch(rows, scale, need_mean, need_value)
            if need_mean:
                shape, dev, dt = ctx.metas[0]
                grad_mean = grad_mean.permute(2, 0, 1).to(device=dev, dtype=dt)  # [B, K, A] over [K][A][B]
            if need_value:
                shape, dev, dt = ctx.metas[1]
                grad_value = grad_value.t().to(device=dev, dtype=dt)
        if need_std:
            shape, dev, dt = ctx.metas[2]
            grad_std = (g * (stats[_native.PPO_STATS:_native.PPO_STATS + A] / n1 - ent_coef)).reshape(shape).to(device=dev, dtype=dt)
        return None, None, None, grad_mean, grad_value, grad_std


class PpoMixin:
    def _ppo_consts(self, log_std, A, fn="vmap_ppo_loss"):
        """log_std [A] -> (log_std in float64 on the device, inv_std [A], logp_const [1]): exp(-log_std) and
        -sum log_std - A/2 log 2 pi, computed in float64 on the device and rounded to the environment's dtype"""
        ls = torch.as_tensor(log_std).detach()
        if tuple(ls.shape) != (A,):
            raise ValueError(f"{fn}: log_std needs to be of shape (action_dim,) which is {(A,)}, but {tuple(ls.shape)} is given")
        ls = ls.to(device=self.device, dtype=torch.float64)
        inv_std = torch.exp(-ls).to(self.dtype)
        const = (-ls.sum() - 0.5 * A * _LOG_2PI).to(self.dtype).reshape(1)
        return ls, inv_std, const

    def _ppo_actions(self, mean, sample, fn):
        """mean, sample [B, K, A] -> (K, A, both over [K][A][B] memory)"""
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        mean, sample = torch.as_tensor(mean), torch.as_tensor(sample)
        if not (mean.ndim == 3 and mean.shape[0] == B and 1 <= mean.shape[2] <= _native.MAX_ACTION):
            raise ValueError(f"{fn}: mean needs to be of shape (batch_size, n_steps, action_dim) with action_dim from 1 to "
                             f"{_native.MAX_ACTION}, but {tuple(mean.shape)} is given")
        K, A = mean.shape[1], mean.shape[2]
        if tuple(sample.shape) != (B, K, A):
            raise ValueError(f"{fn}: sample needs to be of the shape of mean which is {(B, K, A)}, but {tuple(sample.shape)} is given")
        lay = ((B, K, A), (1, A * sB, sB))
        return K, A, cotangent(mean, dev, dt, *lay), cotangent(sample, dev, dt, *lay)

    def vmap_gaussian_logp(self, mean, sample, log_std):
        """Log-probabilities of `sample` under the diagonal Gaussian N(mean, exp(log_std)^2) -> [B, K], a view over [K][B] memory, in
        ONE excenv_gaussian_logp call (include/excenv.h): gaussian_logp_kernel. The collection-time pass of a PPO iteration.

        mean, sample [B, K, A] (A from 1 to 2), log_std [A]. `mean` is what the collection applied, e.g.
        `vmap_policy_eval(policy, ro.observations, n_rows=K)`, and `sample` the PRE-clamp action `noise + mean` (the clamp is part of
        the environment, not of the density). With inv_std = exp(-log_std) and c = -sum log_std - A/2 log 2 pi, both computed in
        float64 and rounded to the environment's dtype:
            z = (sample - mean) * inv_std;   logp = c, then logp = fma(-0.5 z[q], z[q], logp) for q = 0 .. A-1
        `vmap_ppo_loss` runs the same instruction sequence, so the likelihood ratio of an unchanged policy is exactly 1.
        Lane-major views are read in place, anything else is copied once. The inputs are read as values and the result carries no
        graph: a `mean` that requires grad under grad mode is a ValueError (the differentiable entry is `vmap_ppo_loss`)."""
        fn = "vmap_gaussian_logp"
        B, dt, dev = self.batch_size, self.dtype, self.device
        if isinstance(mean, torch.Tensor) and mean.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{fn}: mean requires grad, and the log-probabilities carry no graph: the differentiable entry is "
                             "vmap_ppo_loss (detach the means of the collection)")
        K, A, mean, sample = self._ppo_actions(mean, sample, fn)
        _, inv_std, const = self._ppo_consts(log_std, A, fn)
        logp = torch.empty((K, B), dtype=dt, device=dev)
        if B > 0 and K > 0:
            call = _native.GaussianLogp(mean.data_ptr(), sample.data_ptr(), inv_std.data_ptr(), const.data_ptr(), A, logp.data_ptr())
            _native._launch("excenv_gaussian_logp", logp, fn, _native.dtype_id(dt), B, K, ctypes.byref(call))
        return logp.t()

    def vmap_ppo_loss(self, mean, sample, log_std, logp_old, advantage, value=None, returns=None, reset=None, clip_eps=0.2,
                      vf_coef=0.5, ent_coef=0.0, adv_norm=None, max_groups=0):
        """The clipped PPO objective on stored rows -> `PpoLoss(loss, policy_loss, value_loss, entropy, approx_kl, clip_fraction, n)`,
        0-dim float64 tensors on the device, from ONE excenv_ppo_loss call (include/excenv.h: ppo_loss_kernel, then
        ppo_loss_reduce_kernel): a deterministic reduction of the rows to a handful of fp64 sums, composed with scalar torch ops.
        There is no host synchronisation, no elementwise torch pass and no temporary of the batch's size.

        mean, sample [B, K, A]; log_std [A]; logp_old, advantage [B, K]; value, returns [B, K] or both None (no value loss); reset
        [B, K] bool or None: samples with `reset` set are no transitions (`vmap_rollout_episodes`' convention) and count nowhere.
        `mean` should come from `vmap_policy_eval(policy, obs, n_rows=K)`: its [K][A][B] memory is read in place and the gradient
        goes back the same way. (A `[:, :K]` slice of K + 1 evaluated rows works too, but autograd then materialises a row-major
        gradient of the K + 1 rows, which is copied once.) `sample` is the pre-clamp action `noise + mean_old`; `logp_old` is
        `vmap_gaussian_logp(mean_old, sample, log_std_old)`. adv_norm: None, or (shift, scale), numbers or 0-dim tensors: the
        advantage enters as (advantage - shift) * scale. Per sample, in the environment's dtype (include/excenv.h has every rounding):
            r = exp(logp - logp_old);   surr = min(r a, clamp(r, 1 - clip_eps, 1 + clip_eps) a)
            policy_loss = -sum surr / n;   value_loss = 0.5 sum (value - returns)^2 / n;   approx_kl = sum ((r - 1) - log r) / n
            clip_fraction = share of r outside the clip range;   entropy = sum log_std + A/2 (1 + log 2 pi)
            loss = policy_loss + vf_coef value_loss - ent_coef entropy
        over the n valid samples (n = 0: every mean is 0). max_groups > 0 caps the workgroups of the reduction (its order of
        summation depends on (B, K, max_groups) only; the same call gives the same bits on every run).

        With grad mode on and any of mean, value, log_std requiring grad, `loss` carries ONE autograd node; the other fields carry
        none. Its backward is ONE excenv_ppo_loss_grad call (ppo_loss_grad_kernel) which writes d loss / d mean as a [B, K, A] view
        over [K][A][B] memory (what `vmap_policy_eval`'s backward reads in place) and d loss / d value as a [B, K] view over [K][B];
        log_std.grad comes from the sums of the forward. A sample with `reset` set gets exactly 0. No second derivatives. sample,
        logp_old, advantage and returns are read as values."""
        fn = "vmap_ppo_loss"
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        clip_eps = _number(clip_eps, "clip_eps", fn, 0.0, 1.0)
        coef = (_number(vf_coef, "vf_coef", fn), _number(ent_coef, "ent_coef", fn))
        if not (isinstance(max_groups, int) and not isinstance(max_groups, bool) and 0 <= max_groups < 2 ** 31):
            raise ValueError(f"{fn}: max_groups needs to be a non-negative integer (0: auto), but {max_groups!r} is given")
        if (value is None) != (returns is None):
            raise ValueError(f"{fn}: value and returns need to be given both or neither")
        if adv_norm is not None and not (isinstance(adv_norm, (tuple, list)) and len(adv_norm) == 2):
            raise ValueError(f"{fn}: adv_norm needs to be None or a (shift, scale) pair, but {adv_norm!r} is given")
        K, A, mean_l, sample_l = self._ppo_actions(mean, sample, fn)
        ls, inv_std, const = self._ppo_consts(log_std, A, fn)
        rows = dict(shape=(B, K, A), mean=mean_l, sample=sample_l, inv_std=inv_std, const=const, log_std=ls, clip_eps=clip_eps,
                    max_groups=max_groups)
        for name, t in (("logp_old", logp_old), ("advantage", advantage), ("value", value), ("returns", returns)):
            if t is not None:
                t = torch.as_tensor(t)
                if tuple(t.shape) != (B, K):
                    raise ValueError(f"{fn}: {name} needs to be of shape (batch_size, n_steps) which is {(B, K)}, but {tuple(t.shape)} "
                                     "is given")
                t = cotangent(t, dev, dt, (B, K), (1, sB))
            rows[name] = t
        rows["reset"] = _lane_flags(reset, "reset", fn, B, K, dev)
        rows["adv_norm"] = None if adv_norm is None else torch.stack([_scalar(v, dev) for v in adv_norm]).to(dt)
        graph = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (mean, value, log_std))
        if graph:
            as_t = lambda t: t if (t is None or isinstance(t, torch.Tensor)) else torch.as_tensor(t)
            return PpoLoss(*_PpoObjective.apply(self, rows, coef, as_t(mean), as_t(value), as_t(log_std)))
        return PpoLoss(*self._ppo_loss_fields(rows, coef))

    def _ppo_record(self, rows):
        B, K, A = rows["shape"]
        return _native.PpoLoss(rows["mean"].data_ptr(), rows["sample"].data_ptr(), rows["inv_std"].data_ptr(), rows["const"].data_ptr(),
                               rows["logp_old"].data_ptr(), rows["advantage"].data_ptr(), _native._ptr(rows["value"]),
                               _native._ptr(rows["returns"]), _native._ptr(rows["reset"]), _native._ptr(rows["adv_norm"]), A,
                               rows["max_groups"], rows["clip_eps"], None, None, 0, None, None, None)

    def _ppo_loss_fields(self, rows, coef):
        """One excenv_ppo_loss call on prepared rows -> the fields of PpoLoss; rows["stats"] keeps the sums"""
        B, K, A = rows["shape"]
        dev = self.device
        vf_coef, ent_coef = coef
        if B > 0 and K > 0:
            stats = torch.empty(_native.PPO_STATS + A, dtype=torch.float64, device=dev)
            nbytes = _native.lib().excenv_ppo_loss_workspace_bytes(B, K, rows["max_groups"])
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            call = self._ppo_record(rows)
            call.stats, call.workspace, call.workspace_bytes = stats.data_ptr(), work.data_ptr(), nbytes
            _native._launch("excenv_ppo_loss", stats, "vmap_ppo_loss", _native.dtype_id(self.dtype), B, K, ctypes.byref(call))
        else:
            stats = torch.zeros(_native.PPO_STATS + A, dtype=torch.float64, device=dev)
        rows["stats"] = stats
        n = stats[0].clone()
        n1 = n.clamp(min=1.0)
        policy_loss, value_loss = -stats[1] / n1, 0.5 * stats[2] / n1
        entropy = rows["log_std"].sum() + 0.5 * A * (1.0 + _LOG_2PI)
        loss = policy_loss + vf_coef * value_loss - ent_coef * entropy
        return loss, policy_loss, value_loss, entropy, stats[3] / n1, stats[4] / n1, n

    def _ppo_loss_grad_launch(self, rows, scale, need_mean, need_value):
        """One excenv_ppo_loss_grad call -> (grad_mean [K, A, B] or None, grad_value [K, B] or None)"""
        B, K, A = rows["shape"]
        dt, dev = self.dtype, self.device
        if need_value and rows["value"] is None:
            raise ValueError("vmap_ppo_loss: value requires grad, but it was not part of the loss")
        grad_mean = torch.empty((K, A, B), dtype=dt, device=dev) if need_mean else None
        grad_value = torch.empty((K, B), dtype=dt, device=dev) if need_value else None
        if B > 0 and K > 0:
            call = self._ppo_record(rows)
            call.grad_scale, call.grad_mean, call.grad_value = scale.data_ptr(), _native._ptr(grad_mean), _native._ptr(grad_value)
            _native._launch("excenv_ppo_loss_grad", scale, "vmap_ppo_loss", _native.dtype_id(dt), B, K, ctypes.byref(call))
        return grad_mean, grad_value
