"""The update step of an on-policy trainer on the rows a rollout stored. Mixed into `CoreEnvironment`
(core_env.py).

`vmap_policy_eval` evaluates an `MLPPolicy` — the actor, or a critic with one output — on stored observation rows in ONE
`excenv_policy_eval` call (include/excenv.h: policy_eval_kernel, the rollout's own network bit for bit), and records one autograd node
whose backward is one `excenv_policy_param_grad` call, so a loss on the evaluated means or values reaches `policy.params.grad`.
`vmap_gae` turns the reward / terminated / reset rows of `vmap_rollout_episodes` and a value row into generalised advantage estimates
and returns in ONE `excenv_gae` call (gae_kernel).

Everything is read lane-major: the views `vmap_sim_ahead_policy` / `vmap_rollout_episodes` / `vmap_policy_eval` returned are read in
place, anything else is copied once. Outputs are plain allocations."""
from __future__ import annotations

import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._reverse import cotangent


class _PolicyEval(torch.autograd.Function):
    """vmap_policy_eval with a graph behind its output: policy.params -> [B, R, A]. Forward is the launch the method always makes;
    backward is one excenv_policy_param_grad call on the saved observation view and the incoming gradient."""

    @staticmethod
    def forward(ctx, env, policy, obs, R, row_stride, params):
        ctx.env, ctx.policy, ctx.R, ctx.row_stride = env, policy, R, row_stride
        ctx.meta = (tuple(params.shape), params.device, params.dtype)
        ctx.save_for_backward(obs)
        return env._policy_eval_launch(policy, obs, R, row_stride).permute(2, 0, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        env, policy, R = ctx.env, ctx.policy, ctx.R
        (obs,) = ctx.saved_tensors
        B, A = env.batch_size, policy.widths[-1]
        sB = B or 1
        g_raw = cotangent(g, env.device, env.dtype, (B, R, A), (1, A * sB, sB))  # [R][A][B] memory, copied once if it is not
        grad = env._policy_param_grad_launch(policy, policy.on(env.device, env.dtype).detach(), obs, g_raw, R, ctx.row_stride, 0)
        shape, dev, dt = ctx.meta
        return None, None, None, None, None, grad.reshape(shape).to(device=dev, dtype=dt)


def _lane_flags(flags, name, fn, B, K, device):
    """Optional [B, K] flags -> bytes over [K][B] memory (read in place when they are laid out so), or None"""
    if flags is None:
        return None
    flags = torch.as_tensor(flags).detach()
    if tuple(flags.shape) != (B, K):
        raise ValueError(f"{fn}: {name} needs to be of shape (batch_size, n_steps) which is {(B, K)}, but {tuple(flags.shape)} is given")
    flags = flags.to(device=device, dtype=torch.bool)
    if tuple(flags.stride()) != (1, B or 1):
        flags = flags.t().contiguous().t()
    return flags


class PolicyEvalMixin:
    def vmap_policy_eval(self, policy, observations, row_stride=1, n_rows=None):
        """The network of `vmap_sim_ahead_policy` on stored observation rows -> [B, R, A], a view over [R][A][B] memory: the raw
        output x^L of `policy` (an `MLPPolicy`; no noise, no clamp) for the rows 0, row_stride, 2 row_stride, .. of `observations`
        [B, N+1, OW]. R = n_rows if given, else N // row_stride + 1 (every action row of a rollout with `row_stride` solver steps per
        action, and the last row). One excenv_policy_eval call (include/excenv.h): policy_eval_kernel, bit for bit what the rollout's
        kernel computed for the same stored row, so `clamp(noise + vmap_policy_eval(...)[:, :K])` equals the rollout's actions and
        a likelihood ratio of the unchanged policy is exactly 1. A critic is an `MLPPolicy` with one output.

        Lane-major views (what the rollouts return) are read in place, anything else is copied once. The result is a plain
        allocation. With grad mode on and `policy.params` requiring grad, ONE autograd node is recorded whose backward is one
        excenv_policy_param_grad call (`vmap_policy_param_grads` on the same rows and the incoming gradient): a loss on the result
        reaches `policy.params.grad` and, with `MLPPolicy.from_torch(module, track=True)`, the module's `.grad`. That backward is
        always the fused entry; `env.policy_param_grads` governs rollouts only. No second derivatives. There is no gradient with
        respect to the rows: `observations` that require grad are a ValueError (detach them)."""
        from ._policy import MLPPolicy

        fn = "vmap_policy_eval"
        assert isinstance(policy, MLPPolicy), f"policy needs to be an MLPPolicy, but {type(policy).__name__} is given"
        if not (isinstance(row_stride, int) and row_stride >= 1):
            raise ValueError(f"{fn}: row_stride needs to be a positive integer, but {row_stride!r} is given")
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        OW, A = policy.widths[0], policy.widths[-1]
        observations = torch.as_tensor(observations)
        if not (observations.ndim == 3 and observations.shape[0] == B and observations.shape[1] >= 1 and observations.shape[2] == OW):
            raise ValueError(f"{fn}: observations need to be of shape (batch_size, n_rows, {OW}) with at least one row, but "
                             f"{tuple(observations.shape)} is given")
        if observations.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{fn}: observations require grad, and there is no gradient with respect to the observation rows "
                             "(detach them)")
        rows = observations.shape[1]
        if n_rows is None:
            R = (rows - 1) // row_stride + 1
        else:
            if not (isinstance(n_rows, int) and n_rows >= 0 and (n_rows == 0 or (n_rows - 1) * row_stride < rows)):
                raise ValueError(f"{fn}: n_rows needs to be an integer from 0 to {(rows - 1) // row_stride + 1} ({rows} rows, "
                                 f"row_stride {row_stride}), but {n_rows!r} is given")
            R = n_rows
        if not (OW <= _native.POLICY_MAX_INPUT and A <= _native.MAX_ACTION):
            raise ValueError(f"{fn}: the policy needs at most {_native.POLICY_MAX_INPUT} inputs and {_native.MAX_ACTION} outputs, but "
                             f"its widths are {policy.widths}")
        obs = cotangent(observations, dev, dt, (B, rows, OW), (1, OW * sB, sB))
        if torch.is_grad_enabled() and policy.params.requires_grad:
            return _PolicyEval.apply(self, policy, obs, R, row_stride, policy.params)
        return self._policy_eval_launch(policy, obs, R, row_stride).permute(2, 0, 1)

    def _policy_eval_launch(self, policy, obs, R, row_stride):
        """One excenv_policy_eval call on lane-major obs ([rows][OW][B] in memory) -> [R, A, B]"""
        B, dt, dev = self.batch_size, self.dtype, self.device
        out = torch.empty((R, policy.widths[-1], B), dtype=dt, device=dev)
        if B == 0 or R == 0:
            return out
        params = policy.on(dev, dt).detach()
        widths = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*policy.widths)
        record = _native.Policy(params.data_ptr(), policy.n_layers, _native.ACTIVATIONS[policy.activation], widths, None, 0.0, 0.0)
        call = _native.PolicyEval(record, obs.data_ptr(), out.data_ptr())
        _native._launch("excenv_policy_eval", out, "vmap_policy_eval", _native.dtype_id(dt), B, R, row_stride, ctypes.byref(call))
        return out

    def vmap_gae(self, reward, value, gamma, lam=0.95, terminated=None, reset=None):
        """Generalised advantage estimates of all batch_size environments in one launch -> (advantages [B, K], returns [B, K]),
        views over [K][B] memory. One excenv_gae call (include/excenv.h): gae_kernel, a backward scan per environment in the
        environment's dtype.

        reward [B, K], value [B, K+1] (the critic on every row, e.g. `vmap_policy_eval(critic, ro.observations)[..., 0]`),
        terminated / reset [B, K] bool or None (never), in `vmap_rollout_episodes`' convention: reward[:, n] and terminated[:, n]
        belong to row n + 1; where reset[:, n] is set, row n is a terminal observation and n -> n + 1 no transition: its advantage is
        0, its return value[:, n], and nothing is carried across it. An episode cut by `truncated` or the step budget bootstraps from
        the value of its terminal observation, a terminated one does not, and row K bootstraps the running episode. With
        g = gamma and gl = gamma * lam, backwards from n = K - 1:
            delta = fma(g, value[n + 1] unless terminated[n], reward[n]) - value[n];  adv[n] = fma(gl, adv[n + 1], delta) (delta alone
            when terminated[n]);  returns[n] = adv[n] + value[n]
        gamma and lam lie in [0, 1]. Lane-major views (what `vmap_rollout_episodes` and `vmap_policy_eval` return) are read in
        place, anything else is copied once. The inputs are read as values: the outputs are plain allocations and carry no graph.
        Advantages are not normalised."""
        fn = "vmap_gae"
        B, dt, dev = self.batch_size, self.dtype, self.device
        sB = B or 1
        for name, v in (("gamma", gamma), ("lam", lam)):
            if not (isinstance(v, (int, float)) and not isinstance(v, bool) and not math.isnan(v) and 0.0 <= v <= 1.0):
                raise ValueError(f"{fn}: {name} needs to be a number in [0, 1], but {v!r} is given")
        reward, value = torch.as_tensor(reward), torch.as_tensor(value)
        if not (reward.ndim == 2 and reward.shape[0] == B):
            raise ValueError(f"{fn}: reward needs to be of shape (batch_size, n_steps), but {tuple(reward.shape)} is given")
        K = reward.shape[1]
        if tuple(value.shape) != (B, K + 1):
            raise ValueError(f"{fn}: value needs to be of shape (batch_size, n_steps + 1) which is {(B, K + 1)}, but "
                             f"{tuple(value.shape)} is given")
        terminated = _lane_flags(terminated, "terminated", fn, B, K, dev)
        reset = _lane_flags(reset, "reset", fn, B, K, dev)
        adv = torch.empty((K, B), dtype=dt, device=dev)
        ret = torch.empty((K, B), dtype=dt, device=dev)
        if B > 0 and K > 0:
            reward = cotangent(reward, dev, dt, (B, K), (1, sB))
            value = cotangent(value, dev, dt, (B, K + 1), (1, sB))
            call = _native.Gae(reward.data_ptr(), value.data_ptr(), _native._ptr(terminated), _native._ptr(reset), float(gamma),
                               float(lam), adv.data_ptr(), ret.data_ptr())
            _native._launch("excenv_gae", adv, fn, _native.dtype_id(dt), B, K, ctypes.byref(call))
        return adv.t(), ret.t()
