"""Policy rollouts: `vmap_sim_ahead_policy` runs a whole horizon in ONE persistent launch of sim_policy_kernel through
`excenv_sim_policy` (include/excenv.h), with every action computed inside the kernel by a small multi-layer perceptron on the
observation row it has just saved, plus an optional pre-sampled exploration row, clamped. Mixed into
`CoreEnvironment` (core_env.py); `MLPPolicy` is the parameter record; what the call shares with `vmap_sim_ahead_feedback`
is _closed_loop.py's. `vmap_rollout_episodes` is the same rollout with rewards, flags, a step budget and resets inside the launch
(sim_episodes_kernel through `excenv_sim_policy_episodes`). Nothing here records a graph: a likelihood-ratio
training loop recomputes log-probabilities from the returned observation rows and actions with torch's own autograd, and
`vmap_sim_ahead_policy(..., differentiable=True)` hands over to the reverse mode of _policy_vjp.py."""
from __future__ import annotations

import collections
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

    def torch_forward(self, rows, params=None):
        """The network as differentiable torch operations: rows [..., d_0] -> [..., d_L], the pre-clamp output without noise.
        `params`: a flat tensor laid out like `self.params` (the default), whose views serve as the weights, so
        `torch.autograd.grad(policy.torch_forward(rows, p), p, g)` is the parameter gradient of the rows."""
        p = self.params if params is None else params
        act = torch.tanh if self.activation == "tanh" else torch.relu
        x, off, L = rows, 0, self.n_layers
        for l, (n, d) in enumerate(zip(self.widths[:-1], self.widths[1:])):
            x = torch.nn.functional.linear(x, p[off:off + d * n].view(d, n), p[off + d * n:off + d * (n + 1)])
            if l < L - 1:
                x = act(x)
            off += d * (n + 1)
        return x

    @classmethod
    def from_torch(cls, module, device=None, dtype=None, track=False):
        """From an `nn.Sequential` of `nn.Linear` layers (with bias) separated by one kind of `nn.Tanh` / `nn.ReLU`; anything else
        is a ValueError that names it. The parameters are copied (detached).

        track=True: `params` is instead a `torch.cat` of the module's live parameters with its graph kept, so a backward through
        `vmap_sim_ahead_policy(..., differentiable=True)` fills the module's `.grad`. It is a SNAPSHOT of the values: an optimiser
        step changes the module, not this tensor — build the policy again after every step."""
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
        policy = cls([m.weight for m in linears], [m.bias for m in linears], activation, device=device, dtype=dtype)
        if track:
            live = torch.cat([t.reshape(-1) for m in linears for t in (m.weight, m.bias)])
            policy.params = live.to(device=policy.params.device, dtype=policy.params.dtype)
        return policy


# what `vmap_rollout_episodes` returns: zero-copy views of lane-major memory (`states` is None without a state trajectory)
EpisodeRollout = collections.namedtuple(
    "EpisodeRollout", "observations states last_state actions reward truncated terminated reset n_resets episode_steps")


class PolicyMixin:
    # excenv_last_launch() of the most recent excenv_sim_policy / excenv_sim_policy_episodes launch of this environment
    last_policy_launch = ""

    def _policy_wants_grad(self, init_state, policy, noise):
        """Does the policy's parameter tensor, the noise or a leaf of the initial physical state require grad?"""
        tensors = [getattr(policy, "params", None), noise] + [getattr(init_state.physical_state, n) for n in self.STATE_FIELDS]
        return any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)

    def _policy_call(self, fn, init_state, policy, noise, n_actions, obs_stepsize, action_stepsize, clip, recording=False):
        """The checks and the excenv_policy_t record both policy launches share -> (record, its tensors to keep alive, K, substeps).
        recording: the forward of the autograd node of _policy_vjp.py, which owns the gradients of these inputs."""
        assert isinstance(policy, MLPPolicy), f"policy needs to be an MLPPolicy, but {type(policy).__name__} is given"
        wants = not recording and self._policy_wants_grad(init_state, policy, noise)
        if not recording and self.differentiable and torch.is_grad_enabled() and (self._param_leaves() or wants):
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
        return record, (params, noise), K, sub

    def vmap_sim_ahead_policy(self, init_state, policy, n_actions, obs_stepsize, action_stepsize, noise=None, clip=(-1.0, 1.0),
                              differentiable=None):
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
        and (differentiable=None, the default) `env.differentiable` with an input or parameter that requires grad (there is no
        reverse mode through this launch).

        differentiable=True: when grad mode is on and `policy.params`, the noise or a leaf of the initial physical state requires
        grad, the call records ONE autograd node (_policy_vjp.py) whose backward is one `vmap_sim_ahead_policy_vjp` call;
        observations, state leaves, last state and actions carry the graph, so a loss through
        `vmap_generate_rew_trunc_term_ahead(states, actions)` under `env.differentiable` reaches `policy.params.grad` (and, with
        `MLPPolicy.from_torch(module, track=True)`, the module's `.grad`). With no input that requires grad the plain path runs.
        Refused then: `store_state_trajectory = False`, static parameters that require grad, the saturated PMSM, per-environment
        properties, graph capture. No second derivatives."""
        fn = "vmap_sim_ahead_policy"
        _closed_loop.refuse_settings(self, fn, "policy")
        if differentiable and torch.is_grad_enabled() and (self._param_leaves() or self._policy_wants_grad(init_state, policy, noise)):
            return self._policy_differentiable(init_state, policy, n_actions, obs_stepsize, action_stepsize, noise, clip)
        return self._policy_launch(fn, init_state, policy, n_actions, obs_stepsize, action_stepsize, noise, clip)

    def _policy_launch(self, fn, init_state, policy, n_actions, obs_stepsize, action_stepsize, noise, clip, recording=False):
        """The one excenv_sim_policy launch behind vmap_sim_ahead_policy (its return value); records no graph."""
        record, _keep, K, sub = self._policy_call(fn, init_state, policy, noise, n_actions, obs_stepsize, action_stepsize, clip,
                                                  recording=recording)
        out, name = _closed_loop.launch(self, "excenv_sim_policy", record, fn, init_state, K, sub, obs_stepsize)
        if name is not None:
            self.last_policy_launch = name
        return out

    def _reset_rows(self, reset_states):
        """`reset_states` of vmap_rollout_episodes as S leaves over [R][B] memory -> (leaves, R). A `State` is one row, a list of
        them R rows, a physical-state tree has leaves [B, R]; only what is not laid out as [R][B] already is copied."""
        B = self.batch_size
        if isinstance(reset_states, (list, tuple)):
            assert len(reset_states) >= 1, "reset_states needs at least one State"
            rows = [[self._t(getattr(s.physical_state, n), (B,)).detach() for s in reset_states] for n in self.STATE_FIELDS]
            return [r[0][None] if len(r) == 1 else torch.stack(r) for r in rows], len(reset_states)
        if hasattr(reset_states, "physical_state"):
            return [self._t(getattr(reset_states.physical_state, n), (B,)).detach()[None] for n in self.STATE_FIELDS], 1
        leaves = [torch.as_tensor(getattr(reset_states, n)).detach() for n in self.STATE_FIELDS]
        R = leaves[0].shape[1] if leaves[0].ndim == 2 else 0
        assert R >= 1 and all(tuple(x.shape) == (B, R) for x in leaves), (
            "reset_states needs to be a State, a list of States or a physical state with leaves of shape (batch_size, n_reset_rows) "
            + f"which is {(B, 'R')}, but {[tuple(x.shape) for x in leaves]} is given")
        return [x.to(device=self.device, dtype=self.dtype).t().contiguous() for x in leaves], R

    def vmap_rollout_episodes(self, init_state, policy, n_actions, stepsize, reset_states, noise=None, clip=(-1.0, 1.0),
                              end_on=("terminated", "truncated"), max_episode_steps=0, episode_steps=None):
        """`vmap_sim_ahead_policy` with the rewards, the flags and the episode boundaries inside the same kernel launch: K = n_actions
        steps of `stepsize` for all batch_size environments -> EpisodeRollout(observations [B, K+1, OW], states with leaves
        [B, K+1] (None with `env.store_state_trajectory = False`), last_state, actions [B, K, A], reward [B, K], truncated
        [B, K+1, TW] bool, terminated [B, K] bool, reset [B, K] bool, n_resets [B] int32, episode_steps [B] int32).

        Row n of an environment is judged as soon as it is saved: the episode ends there when `terminated` / `truncated` (those named
        in `end_on`) is set for the row's state, or when the running episode already has `max_episode_steps` steps (0: no limit;
        `episode_steps` [B] gives the steps taken before this call, None: zeros). Then reset[:, n] is True, the action of row n is
        computed and returned but not applied, and row n + 1 is the environment's next reset state: row (e mod R) of `reset_states`
        at its e-th reset within the call. Otherwise row n + 1 is `vmap_step`'s result, bit for bit. Row n with reset[:, n] is the
        terminal observation and row n + 1 the first one of the next episode (gymnasium's "next-step" convention): a trainer masks the
        transitions with reset[:, n]. Row 0 is judged like every other row; its `terminated` value has no slot, reset[:, 0] shows the
        verdict. reward[:, n - 1] / terminated[:, n - 1] / truncated[:, n] belong to row n and are pure functions of it, reset rows
        included: bit for bit `vmap_generate_rew_trunc_term_ahead(states, actions)`. References stay as they are along the call; a
        reset state that is itself terminal resets again one step later.

        reset_states: a `State` (from `vmap_reset` / `vmap_init_state`: R = 1), a list of them, or a physical state with leaves
        [B, R]. Without a `control_state` the reward of every model but the PMSM is 0 and its `terminated` is `reward == 0` in every
        row (the reference's semantics): "terminated" in `end_on` then resets on every step, `end_on=("truncated",)` is the usual
        choice there. episode_steps of the result carries over to the next call.

        No recording form: `vmap_sim_ahead_policy_vjp(policy, observations, states, actions, ..., reset=result.reset)` is the route
        to gradients. Refused by name (ValueError): what `vmap_sim_ahead_policy` refuses, an unknown `end_on` entry, and `end_on=()` with
        `max_episode_steps=0` (nothing can end an episode: that is `vmap_sim_ahead_policy`)."""
        fn = "vmap_rollout_episodes"
        _closed_loop.refuse_settings(self, fn, "episode")
        mask = 0
        for name in end_on:
            if name not in _native.END_ON:
                raise ValueError(f"{fn}: end_on entry {name!r}: 'terminated' or 'truncated'")
            mask |= _native.END_ON[name]
        max_episode_steps = int(max_episode_steps)
        assert 0 <= max_episode_steps < 2 ** 31, f"max_episode_steps needs to be a non-negative int32, but {max_episode_steps} is given"
        if mask == 0 and max_episode_steps == 0:
            raise ValueError(f"{fn}: end_on=() and max_episode_steps=0: nothing can end an episode; that is vmap_sim_ahead_policy")
        record, _keep, K, _sub = self._policy_call(fn, init_state, policy, noise, n_actions, stepsize, stepsize, clip)
        B, dev = self.batch_size, self.device
        rows, R = self._reset_rows(reset_states)
        steps_in = None
        if episode_steps is not None:
            steps_in = torch.as_tensor(episode_steps).detach().to(device=dev, dtype=torch.int32).contiguous()
            assert tuple(steps_in.shape) == (B,), (
                f"episode_steps needs to be of shape (batch_size,) which is {(B,)}, but {tuple(steps_in.shape)} is given")
        TW = _native.truncated_width(self.ENV_ID, len(self.control_state))
        rew = torch.empty((K, B), dtype=self.dtype, device=dev)
        term = torch.empty((K, B), dtype=torch.bool, device=dev)
        trunc = torch.empty((K + 1, B, TW), dtype=torch.bool, device=dev)
        reset = torch.empty((K, B), dtype=torch.bool, device=dev)
        n_resets = torch.zeros(B, dtype=torch.int32, device=dev)
        steps_out = torch.zeros(B, dtype=torch.int32, device=dev)
        row_ptrs = _native._ptrs(rows)  # (alive until the launch is enqueued)
        episode = _native.Episode(ctypes.addressof(row_ptrs), R, mask, max_episode_steps, _native._ptr(steps_in),
                                  rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), reset.data_ptr(), n_resets.data_ptr(),
                                  steps_out.data_ptr())
        (obs, states, last, actions), name = _closed_loop.launch(self, "excenv_sim_policy_episodes", record, fn, init_state, K, 1, stepsize,
                                                                 extra=(ctypes.byref(episode),))
        if name is not None:
            self.last_policy_launch = name
        return EpisodeRollout(obs, states, last, actions, rew.t(), trunc.permute(1, 0, 2), term.t(), reset.t(), n_resets, steps_out)
