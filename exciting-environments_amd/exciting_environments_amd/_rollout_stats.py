"""Rollout statistics on the rows a rollout stored. Mixed into `CoreEnvironment` (core_env.py), next to `PpoMixin`.

`vmap_row_moments` is ONE `excenv_row_moments` call (include/excenv.h: row_moments_kernel and its reduction): the masked count, sums and
sums of squares of up to 16 columns as a handful of fp64 numbers, from which mean and variance are composed with scalar torch ops.
`vmap_advantage_norm` is that call on the advantages and gives the `(shift, scale)` pair `vmap_ppo_loss(adv_norm=...)` takes.
`vmap_episode_stats` is ONE `excenv_episode_stats` call (episode_stats_kernel and the same reduction): the returns and lengths of the
episodes a rollout finished, with the two per-environment carries that continue the running episodes in the next call.
`RunningMoments` merges `RowMoments` across iterations (what observation normalisation needs).

Everything is read lane-major: the views the rollouts and `vmap_gae` returned are read in place, anything else is copied once. Outputs
are plain allocations. The inputs are read as values and the results carry no graph. Nothing here synchronises with the host."""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import torch

from . import _native
from ._policy_eval import _lane_flags
from ._reverse import cotangent

RowMoments = namedtuple("RowMoments", ["n", "mean", "var", "sum", "sumsq"])
RowMoments.__doc__ = """What `vmap_row_moments` returns: float64 tensors on the environment's device. `n` (0-dim) is the number of valid
samples; `mean`, `var` [C] are the moments of the columns; `sum`, `sumsq` [C] are the kernel's sums S1, S2 of (x - shift) and its
square."""

EpisodeStats = namedtuple("EpisodeStats", ["n_episodes", "mean_return", "std_return", "mean_length", "min_return", "max_return",
                                           "episode_return", "episode_steps", "completed"])
EpisodeStats.__doc__ = """What `vmap_episode_stats` returns. The first six are 0-dim float64 tensors on the environment's device over the
episodes the rows finished (`n_episodes` == 0: the means and the deviation are 0, `min_return` is +inf and `max_return` -inf;
`std_return` is the population deviation). `episode_return` [B] float64 and `episode_steps` [B] int32 are the carries of the running
episodes: pass them to the next call. `completed` is None, or with per_row=True a [B, K] float64 view over [K][B] memory that holds the
return of the episode that ended at that row and 0 elsewhere."""


def _lane_rows(t, name, fn, device, dtype, shape, strides):
    """`t` of `shape` over lane-major memory (`strides`) on the device in the working dtype: itself when it is laid out so, wherever it
    starts (the kernels take element accesses then), else one copy"""
    t = torch.as_tensor(t).detach()
    if tuple(t.shape) != shape:
        raise ValueError(f"{fn}: {name} needs to be of shape {shape}, but {tuple(t.shape)} is given")
    if t.device == device and t.dtype == dtype and tuple(t.stride()) == strides:
        return t
    return cotangent(t, device, dtype, shape, strides)


def _count(v, name, fn, hi=2 ** 31):
    if not (isinstance(v, int) and not isinstance(v, bool) and 0 <= v < hi):
        raise ValueError(f"{fn}: {name} needs to be a non-negative integer, but {v!r} is given")
    return v


class RolloutStatsMixin:
    def vmap_row_moments(self, x, mask=None, shift=None, ddof=0, max_groups=0):
        """Masked moments of the columns of stored rows -> `RowMoments(n, mean, var, sum, sumsq)`, float64 tensors on the device (`n`
        0-dim, the others [C]), from ONE excenv_row_moments call (include/excenv.h: row_moments_kernel, then
        rollout_stats_reduce_kernel): a deterministic reduction to 1 + 2 C fp64 sums, composed with scalar torch ops. There is no host
        synchronisation, no boolean index, no elementwise torch pass and no temporary of the batch's size.

        x [B, N] (C = 1) or [B, N, C] with C from 1 to 16: advantages, rewards, or the observation rows of a rollout (a [B, N, C] view
        over [N][C][B] memory is read in place). mask [B, N] bool or None: samples with `mask` set are excluded (for the rows of
        `vmap_rollout_episodes`: its `reset`); whatever they hold, a NaN included, reaches nothing. shift: None, or [C] numbers or a
        tensor (a number for C = 1): the sums are taken of x - shift in float64, which keeps the variance of a column far from zero
        well conditioned; any value near the column's mean serves, e.g. its first element or last iteration's mean. With n' = max(n, 1):
            mean = shift + S1 / n';   var = max(0, (S2 - S1^2 / n') / max(n - ddof, 1))
        so an all-masked call gives n = 0, mean = shift and var = 0. max_groups > 0 caps the workgroups of the reduction (its order of
        summation depends on (B, N, C, max_groups) only; the same call gives the same bits on every run)."""
        fn = "vmap_row_moments"
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        max_groups = _count(max_groups, "max_groups", fn)
        if not (isinstance(ddof, (int, float)) and not isinstance(ddof, bool) and math.isfinite(ddof) and ddof >= 0):
            raise ValueError(f"{fn}: ddof needs to be a non-negative number, but {ddof!r} is given")
        x = torch.as_tensor(x)
        if not (x.ndim in (2, 3) and x.shape[0] == B):
            raise ValueError(f"{fn}: x needs to be of shape (batch_size, n_rows) or (batch_size, n_rows, n_columns) with batch_size "
                             f"{B}, but {tuple(x.shape)} is given")
        N, C = x.shape[1], (x.shape[2] if x.ndim == 3 else 1)
        if not 1 <= C <= _native.MOMENTS_MAX_COLUMNS:
            raise ValueError(f"{fn}: x needs to have from 1 to {_native.MOMENTS_MAX_COLUMNS} columns, but {tuple(x.shape)} is given")
        if x.ndim == 2:
            rows = _lane_rows(x, "x", fn, dev, dt, (B, N), (1, sB))
        else:
            rows = _lane_rows(x, "x", fn, dev, dt, (B, N, C), (1, C * sB, sB))
        flags = _lane_flags(mask, "mask", fn, B, N, dev)
        if shift is None:
            shift_t = None
        else:
            # (numbers are taken as float64: torch's default for a list of Python floats is float32)
            shift_t = shift.detach() if isinstance(shift, torch.Tensor) else torch.as_tensor(shift, dtype=torch.float64)
            shape = tuple(shift_t.shape)
            shift_t = shift_t.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
            if shift_t.numel() != C:
                raise ValueError(f"{fn}: shift needs to hold one number per column which is {C}, but {shape} is given")
        if B > 0 and N > 0:
            stats = torch.empty(1 + 2 * C, dtype=torch.float64, device=dev)
            nbytes = _native.lib().excenv_row_moments_workspace_bytes(B, N, C, max_groups)
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            call = _native.RowMoments(rows.data_ptr(), _native._ptr(flags), _native._ptr(shift_t), C, max_groups, stats.data_ptr(),
                                      work.data_ptr(), nbytes)
            _native._launch("excenv_row_moments", stats, fn, _native.dtype_id(dt), B, N, ctypes.byref(call))
        else:
            stats = torch.zeros(1 + 2 * C, dtype=torch.float64, device=dev)
        n = stats[0].clone()
        n1 = n.clamp(min=1.0)
        s1, s2 = stats[1:1 + C], stats[1 + C:]
        mean = s1 / n1 if shift_t is None else shift_t + s1 / n1
        var = ((s2 - s1 * s1 / n1) / (n - float(ddof)).clamp(min=1.0)).clamp(min=0.0)
        return RowMoments(n, mean, var, s1, s2)

    def vmap_advantage_norm(self, advantage, reset=None, eps=1e-8, ddof=1):
        """The advantage normalisation of a PPO update -> `(shift, scale)` = (mean, 1 / (sqrt(var) + eps)) of the advantages of the
        valid samples, 0-dim float64 tensors on the device: what `vmap_ppo_loss(adv_norm=...)` takes. ONE excenv_row_moments call
        (`vmap_row_moments` with the advantages as the one column and `reset` as the mask) and a few scalar torch ops; no host
        synchronisation.

        advantage [B, K] (`vmap_gae`'s view is read in place); reset [B, K] bool or None: the samples `vmap_ppo_loss` leaves out. ddof
        = 1 is torch.std's default. No valid sample: shift 0 and scale 1 / eps."""
        fn = "vmap_advantage_norm"
        if not (isinstance(eps, (int, float)) and not isinstance(eps, bool) and math.isfinite(eps) and eps > 0):
            raise ValueError(f"{fn}: eps needs to be a positive number, but {eps!r} is given")
        adv = torch.as_tensor(advantage)
        if adv.ndim != 2:
            raise ValueError(f"{fn}: advantage needs to be of shape (batch_size, n_steps), but {tuple(adv.shape)} is given")
        m = self.vmap_row_moments(adv, mask=reset, ddof=ddof)
        return m.mean[0], 1.0 / (torch.sqrt(m.var[0]) + float(eps))

    def vmap_episode_stats(self, reward, reset, episode_return=None, episode_steps=None, per_row=False):
        """Returns and lengths of the episodes the rows of `vmap_rollout_episodes` finished -> `EpisodeStats(n_episodes, mean_return,
        std_return, mean_length, min_return, max_return, episode_return, episode_steps, completed)` from ONE excenv_episode_stats call
        (include/excenv.h: episode_stats_kernel, then rollout_stats_reduce_kernel); no host synchronisation, no scan in torch.

        reward, reset [B, K]: `ro.reward` and `ro.reset`, read in place. In the rollout's convention reward[n] belongs to row n + 1 and
        reset[n] says that the episode ended at row n, so transition n is no step and its reward is dropped. Per environment, in
        float64, with ret = episode_return (0 where None) and len = episode_steps (0 where None):
            reset[n]:  an episode of len > 0 steps is finished with return ret (len == 0 is no episode);  ret = 0;  len = 0
            else:      ret += reward[n];  len += 1
        episode_return [B] (float64) and episode_steps [B] (int32) are the carries of the running episodes: pass the returned ones to
        the next call, and the `episode_steps` the rollout was given to the first. The returned counter then equals the rollout's
        `ro.episode_steps`. per_row=True also returns `completed` [B, K] (the return of the episode that ended at that row, 0 elsewhere).
        The statistics are undiscounted."""
        fn = "vmap_episode_stats"
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        reward = torch.as_tensor(reward)
        if not (reward.ndim == 2 and reward.shape[0] == B):
            raise ValueError(f"{fn}: reward needs to be of shape (batch_size, n_steps) with batch_size {B}, but {tuple(reward.shape)} "
                             "is given")
        K = reward.shape[1]
        if reset is None:
            raise ValueError(f"{fn}: reset is needed: the [B, K] flags vmap_rollout_episodes returned")
        rows = _lane_rows(reward, "reward", fn, dev, dt, (B, K), (1, sB))
        flags = _lane_flags(reset, "reset", fn, B, K, dev)
        carries = []
        for name, t, cdt in (("episode_return", episode_return, torch.float64), ("episode_steps", episode_steps, torch.int32)):
            if t is not None:
                t = t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=cdt)
                if tuple(t.shape) != (B,):
                    raise ValueError(f"{fn}: {name} needs to be of shape (batch_size,) which is {(B,)}, but {tuple(t.shape)} is given")
                t = t.to(device=dev, dtype=cdt).contiguous()
            carries.append(t)
        ret_in, steps_in = carries
        ret_out = torch.empty(B, dtype=torch.float64, device=dev)
        steps_out = torch.empty(B, dtype=torch.int32, device=dev)
        completed = torch.empty((K, B), dtype=torch.float64, device=dev) if per_row else None
        if B > 0 and K > 0:
            stats = torch.empty(_native.EPISODE_STATS, dtype=torch.float64, device=dev)
            nbytes = _native.lib().excenv_episode_stats_workspace_bytes(B)
            work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            call = _native.EpisodeStats(rows.data_ptr(), flags.data_ptr(), _native._ptr(ret_in), _native._ptr(steps_in),
                                        _native._ptr(completed), ret_out.data_ptr(), steps_out.data_ptr(), stats.data_ptr(),
                                        work.data_ptr(), nbytes)
            _native._launch("excenv_episode_stats", stats, fn, _native.dtype_id(dt), B, K, ctypes.byref(call))
        else:
            stats = torch.tensor([0.0, 0.0, 0.0, 0.0, math.inf, -math.inf], dtype=torch.float64, device=dev)
            ret_out = torch.zeros(B, dtype=torch.float64, device=dev) if ret_in is None else ret_in.clone()
            steps_out = torch.zeros(B, dtype=torch.int32, device=dev) if steps_in is None else steps_in.clone()
        n = stats[0].clone()
        n1 = n.clamp(min=1.0)
        mean = stats[1] / n1
        std = torch.sqrt(((stats[2] - stats[1] * stats[1] / n1) / n1).clamp(min=0.0))
        return EpisodeStats(n, mean, std, stats[3] / n1, stats[4].clone(), stats[5].clone(), ret_out, steps_out,
                            None if completed is None else completed.t())


class RunningMoments:
    """Moments of everything a sequence of `RowMoments` saw, merged by Chan's parallel formula on [C] float64 tensors:
        n = n_a + n_b;  delta = mean_b - mean_a;  mean = mean_a + delta n_b / n;  M2 = M2_a + M2_b + delta^2 n_a n_b / n
    with M2_b = S2 - S1^2 / n_b of the chunk (shift-invariant, so chunks taken with different shifts merge). Torch ops on a few numbers
    only: no host synchronisation, whatever device the moments live on. A chunk without a valid sample changes nothing.

    This is what observation normalisation needs: `rm.update(env.vmap_row_moments(ro.observations, mask=...))` every iteration, then
    `rm.mean` and `rm.std()`. Folding (obs - mean) / std into a policy's first layer (W' = W / std, b' = b - W' mean) is left to the
    caller: the rollout kernels read raw observations."""

    def __init__(self):
        self.n = self.mean = self.m2 = None

    def update(self, moments):
        """Merge one `RowMoments` -> self"""
        nb = moments.n.detach()
        nb1 = nb.clamp(min=1.0)
        mean_b = moments.mean.detach()
        m2_b = (moments.sumsq.detach() - moments.sum.detach() ** 2 / nb1).clamp(min=0.0)
        if self.n is None:
            self.n, self.mean, self.m2 = nb.clone(), torch.where(nb > 0, mean_b, torch.zeros_like(mean_b)), m2_b
            return self
        if tuple(mean_b.shape) != tuple(self.mean.shape):
            raise ValueError(f"RunningMoments.update: moments of {tuple(mean_b.shape)} columns, but {tuple(self.mean.shape)} were merged before")
        n = self.n + nb
        n1 = n.clamp(min=1.0)
        delta = torch.where(nb > 0, mean_b - self.mean, torch.zeros_like(mean_b))
        self.mean = self.mean + delta * (nb / n1)
        self.m2 = self.m2 + m2_b + delta * delta * (self.n * nb / n1)
        self.n = n
        return self

    def var(self, ddof=0):
        """[C]: M2 / max(n - ddof, 1)"""
        return self.m2 / (self.n - float(ddof)).clamp(min=1.0)

    def std(self, eps=0.0, ddof=0):
        """[C]: sqrt(var) + eps"""
        return torch.sqrt(self.var(ddof)) + float(eps)
