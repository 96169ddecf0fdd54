"""Policy rollouts: `vmap_sim_ahead_policy` runs a whole horizon in ONE persistent launch of sim_policy_kernel through
`excenv_sim_policy` (include/excenv.h), with every action computed inside the kernel by a small multi-layer perceptron on the
observation row it has just saved, plus an optional pre-sampled exploration row, clamped. Mixed into
`CoreEnvironment` (core_env.py); `MLPPolicy` is the parameter record; what the call shares with `vmap_sim_ahead_feedback`
is _closed_loop.py's. Nothing here records a graph: a training loop recomputes log-probabilities from the returned observation
rows and actions with torch's own autograd."""
from __future__ import annotations

import ctypes

import torch

from . import _closed_loop, _native


class MLPPolicy:
    """The parameters of a multi-layer perceptron policy: `weights[l]` of shape [d_{l+1}, d_l] (torch's nn.Linear.weight layout),
    `biases[l]` of shape [d_{l+1}], one activation ("tanh" or "relu") behind every layer but the last. At most 4 linear layers,
    hidden widths 1 .. 64; the first width is the environment's observation width, the last its action width.

    Holds ONE flat tensor `params` — W_1, b_1, .., W_L, b_L, each row-major — which the kernel reads in place; `on(device, dtype)`
    gives it on an environment's device in its dtype (converted once and kept)."""

    def __init__(self, weights, biases, activation="tanh", device=None, dtype=None):
        if activation not in _native.ACTIVATIONS:
            raise ValueError(f"MLPPolicy: activation={activation!r}: 'tanh' or 'relu'")
        weights = [torch.as_tensor(w).detach() for w in weights]
        biases = [torch.as_tensor(b).detach() for b in biases]
        assert len(weights) == len(biases) and 1 <= len(weights) <= _native.POLICY_MAX_LAYERS, (
            f"MLPPolicy needs 1 to {_native.POLICY_MAX_LAYERS} linear layers with one bias each, but {len(weights)} weights and "
            f"{len(biases)} biases are given")
        widths = []
        for l, (w, b) in enumerate(zip(weights, biases)):
            assert w.ndim == 2 and b.ndim == 1 and b.shape[0] == w.shape[0], (
                f"MLPPolicy: layer {l + 1} needs a weight (out, in) and a bias (out,), but {tuple(w.shape)} and {tuple(b.shape)} are given")
            assert not widths or widths[-1] == w.shape[1], (
                f"MLPPolicy: layer {l + 1} reads {w.shape[1]} inputs, but layer {l} has {widths[-1] if widths else 0} outputs")
            if not widths:
                widths.append(int(w.shape[1]))
            widths.append(int(w.shape[0]))
        for l in range(1, len(widths) - 1):
            assert 1 <= widths[l] <= _native.POLICY_MAX_WIDTH, (
                f"MLPPolicy: hidden layer {l} has {widths[l]} units; 1 to {_native.POLICY_MAX_WIDTH} are supported")
        self.widths = tuple(widths)
        self.activation = activation
        dtype = dtype or weights[0].dtype
        device = device or weights[0].device
        self.params = torch.cat([t.to(device=device, dtype=dtype).reshape(-1) for pair in zip(weights, biases) for t in pair])
        self._placed = {}

    @property
    def n_layers(self):
        return len(self.widths) - 1

    def on(self, device, dtype):
        """The flat parameter tensor on `device` in `dtype`"""
        device = torch.device(device)
        if self.params.device == device and self.params.dtype == dtype:
            return self.params
        key = (device, dtype)
        if key not in self._placed:
            self._placed[key] = self.params.to(device=device, dtype=dtype).contiguous()
        return self._placed[key]

    def layers(self):
        """[(W_l [d_l, d_{l-1}], b_l [d_l])]: views of `params`"""
        out, off = [], 0
        for n, d in zip(self.widths[:-1], self.widths[1:]):
            out.append((self.params[off:off + d * n].view(d, n), self.params[off + d * n:off + d * (n + 1)]))
            off += d * (n + 1)
        return out

    @classmethod
    def from_torch(cls, module, device=None, dtype=None):
        """From an `nn.Sequential` of `nn.Linear` layers (with bias) separated by one kind of `nn.Tanh` / `nn.ReLU`; anything else
        is a ValueError that names it. The parameters are copied (detached)."""
        nn = torch.nn
        if not isinstance(module, nn.Sequential):
            raise ValueError(f"MLPPolicy.from_torch: needs an nn.Sequential of Linear layers, got {type(module).__name__}")
        mods = list(module)
        if len(mods) % 2 == 0:
            raise ValueError("MLPPolicy.from_torch: needs Linear (activation Linear)*: a Linear layer first and last, "
                             f"got {[type(m).__name__ for m in mods]}")
        kinds = set()
        for j, m in enumerate(mods):
            if j % 2 == 0:
                if not isinstance(m, nn.Linear):
                    raise ValueError(f"MLPPolicy.from_torch: module {j} must be nn.Linear, got {type(m).__name__}")
                if m.bias is None:
                    raise ValueError(f"MLPPolicy.from_torch: module {j}: nn.Linear(bias=False) is not supported")
            else:
                if type(m) not in (nn.Tanh, nn.ReLU):
                    raise ValueError(f"MLPPolicy.from_torch: module {j} must be nn.Tanh or nn.ReLU, got {type(m).__name__}")
                kinds.add(type(m))
        if len(kinds) > 1:
            raise ValueError("MLPPolicy.from_torch: nn.Tanh and nn.ReLU mixed: one activation serves all hidden layers")
        linears = mods[0::2]
        if len(linears) > _native.POLICY_MAX_LAYERS:
            raise ValueError(f"MLPPolicy.from_torch: {len(linears)} Linear layers; at most {_native.POLICY_MAX_LAYERS} are supported")
        for j, m in enumerate(linears[:-1]):
            if not 1 <= m.out_features <= _native.POLICY_MAX_WIDTH:
                raise ValueError(f"MLPPolicy.from_torch: hidden layer {j + 1} has {m.out_features} units; 1 to "
                                 f"{_native.POLICY_MAX_WIDTH} are supported")
        activation = "relu" if nn.ReLU in kinds else "tanh"
        return cls([m.weight for m in linears], [m.bias for m in linears], activation, device=device, dtype=dtype)


class PolicyMixin:
    # excenv_last_launch() of the most recent excenv_sim_policy launch of this environment
    last_policy_launch = ""

    def vmap_sim_ahead_policy(self, init_state, policy, n_actions, obs_stepsize, action_stepsize, noise=None, clip=(-1.0, 1.0)):
        """Rollouts of all batch_size environments under an MLP policy in one kernel launch -> (observations [B, N+1, OW], states
        with leaves [B, N+1], last_state with leaves [B], actions [B, K, A]), K = n_actions action rows of substeps = action_stepsize
        / obs_stepsize solver steps each, N = K * substeps.

        At every action row k the kernel reads the observation row it has just saved (row k * substeps, the normalised references
        of `control_state` included: what `generate_observation` builds), evaluates `policy` (an `MLPPolicy`: sums as fused
        multiply-adds in input order, the activation behind every layer but the last) and applies
            a[k] = clamp(noise[k] + mlp(obs_row))
        for `substeps` steps of `vmap_step`'s arithmetic.

        noise: [B, K, A] pre-sampled exploration (e.g. sigma * randn) or None; a view from `env.new_actions_buffer(K)` is read in
        place, anything else is copied into one. n_actions may be None when `noise` gives it. clip: (low, high), None: no clamp.

        The returned tensors are views of freshly allocated lane-major memory and carry no graph; `states` is None with
        `env.store_state_trajectory = False`. `vmap_generate_rew_trunc_term_ahead(states, actions)` gives the gym outputs.
        Refused by name (ValueError): trajectory layouts other than "lane_major", `sim_ahead_semantics == "ahead_accumulated_t"`,
        and `env.differentiable` with an input or parameter that requires grad (there is no reverse mode through this launch)."""
        fn = "vmap_sim_ahead_policy"
        _closed_loop.refuse_settings(self, fn, "policy")
        assert isinstance(policy, MLPPolicy), f"policy needs to be an MLPPolicy, but {type(policy).__name__} is given"
        tensors = [policy.params, noise] + [getattr(init_state.physical_state, n) for n in self.STATE_FIELDS]
        wants = any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)
        if self.differentiable and torch.is_grad_enabled() and (self._param_leaves() or wants):
            raise ValueError(f"{fn}: env.differentiable with an input that requires grad: there is no reverse mode through the policy "
                             "launch; detach the inputs or set env.differentiable = False, and recompute the log-probabilities from "
                             "the returned observations and actions in torch")
        A, OW = self.action_dim, self._obs_dim()
        _closed_loop.check_state(self, init_state, obs_stepsize, action_stepsize)
        assert policy.widths[0] == OW and policy.widths[-1] == A, (
            f"The policy needs to map the observation width {OW} to the action width {A}, but its widths are {policy.widths}")
        noise, K = _closed_loop.action_rows(self, noise, "noise", n_actions)
        sub = self._n_substeps(K, obs_stepsize, action_stepsize)
        lo, hi = _closed_loop.clip_bounds(clip)
        noise = _closed_loop.lane_major_rows(self, noise, K)
        params = policy.on(self.device, self.dtype)
        widths = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*policy.widths)
        record = _native.Policy(params.data_ptr(), policy.n_layers, _native.ACTIVATIONS[policy.activation], widths,
                                _native._ptr(noise) if K > 0 else None, lo, hi)
        out, name = _closed_loop.launch(self, "excenv_sim_policy", record, fn, init_state, K, sub, obs_stepsize)
        if name is not None:
            self.last_policy_launch = name
        return out
