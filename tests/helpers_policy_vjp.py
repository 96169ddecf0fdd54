"""The float64 torch twin of the policy rollout's reverse mode (tests/test_policy_vjp_host.py, tests/test_gpu_policy_vjp.py):
helpers_feedback_vjp.twin_step and helpers_vjp.Twin's observe with a torch multi-layer perceptron and helpers_vjp.clamp0 (derivative 0
on and outside the bounds; torch's ReLU has derivative 0 at 0, the kernel's convention). Gradients come from torch.autograd.grad on
the CPU.

The twin records, per environment, the smallest distance of a pre-clamp output to a clamp bound (relative to the clamp's width, as
helpers_feedback_vjp.closed_loop's bound_distance; it joins Twin.kinks, so one mask covers the model's kinks and the clamp) and the
smallest absolute ReLU pre-activation (`relu_min`, its own margin).

Inputs are helpers_policy.policy_inputs'; the main case is B_MAIN = 326, K_MAIN = 7, substeps 3 (PMSM: 1)."""
import functools

import numpy as np
import torch

import helpers_policy as hp
from helpers_feedback import B_MAIN, CLIP, K_MAIN, substeps_of  # noqa: F401
from helpers_feedback_vjp import twin_step
from helpers_vjp import DT, KINK_CAP, KINK_MARGIN, Twin, clamp0, normalize  # noqa: F401  (the caps: for the tests)

RELU_MARGIN = 3e-5       # fp32: environments with a ReLU pre-activation closer to 0 than this are excluded
RELU_MARGIN_FP64 = 1e-6  # fp64 comparisons of ReLU networks


def torch_mlp(x, W, b, activation, pre=None):
    """x [B, d_0] -> x^L [B, d_L]; pre: a list that receives the hidden pre-activations (detached)"""
    L = len(W)
    for l in range(L):
        x = x @ W[l].t() + b[l]
        if l < L - 1:
            if pre is not None:
                pre.append(x.detach())
            x = torch.tanh(x) if activation == "tanh" else torch.relu(x)
    return x


def policy_loop(twin, st, W, b, activation, noise, K, sub, clip, tau, refs=None, control=None, reset=None, reset_rows=None):
    """st: list of S [B] tensors; W / b: the layers as tensors; noise [B, K, A] or None; refs: {field: [B] array} of the controlled
    fields `control`. reset [B, K] bool with reset_rows (S x [B, K+1] constants, sub == 1): where reset[:, n], row n + 1 is
    reset_rows[:, n + 1] instead of the step's result (torch.where on the mask) -> dict(obs [B, N+1, OW], states (S x [B, N+1]),
    last (S x [B]), actions [B, K, A], relu_min [B] (inf without ReLU units), clamped: share of action entries on the clamp)"""
    twin.kinks, twin.clips, twin.levels = [], [], []
    B = st[0].shape[0]
    A = W[-1].shape[0]
    lo, hi = (-np.inf, np.inf) if clip is None else (float(clip[0]), float(clip[1]))
    cref = []
    for name in (control or []):
        j = twin.fields.index(name)
        cref.append(normalize(torch.as_tensor(np.asarray(refs[name], np.float64), dtype=DT), twin.smin[j], twin.smax[j]))

    def observe(s):
        ob = twin.observe(s)
        return torch.cat([ob] + [c[:, None] for c in cref], dim=1) if cref else ob

    relu_min = torch.full((B,), np.inf, dtype=DT)
    st = list(st)
    rows, obs_rows, acts = [], [], []
    n_clamped = 0
    for k in range(K):
        ob = observe(st)
        pre = []
        raw = torch_mlp(ob, W, b, activation, pre)
        if noise is not None:
            raw = noise[:, k] + raw
        if activation == "relu":
            for p in pre:
                relu_min = torch.minimum(relu_min, p.abs().min(dim=1).values)
        if clip is not None:
            d = torch.minimum((raw.detach() - lo).abs(), (raw.detach() - hi).abs()) / (hi - lo)
            twin.kinks.append(d.min(dim=1).values)
        n_clamped += int(((raw.detach() <= lo) | (raw.detach() >= hi)).sum())
        a = clamp0(raw, lo, hi)
        acts.append(a)
        for s in range(sub):
            rows.append(list(st))
            obs_rows.append(ob if s == 0 else observe(st))
            nxt = twin_step(twin, st, [a[:, q] for q in range(A)], float(tau))
            if reset is not None:
                m = torch.as_tensor(np.asarray(reset[:, k]), dtype=torch.bool)
                nxt = [torch.where(m, torch.as_tensor(np.asarray(r[:, k + 1], np.float64), dtype=DT), x) for x, r in zip(nxt, reset_rows)]
            st = nxt
    rows.append(list(st))
    obs_rows.append(observe(st))
    S = len(st)
    return dict(obs=torch.stack(obs_rows, dim=1), states=[torch.stack([r[j] for r in rows], dim=1) for j in range(S)], last=st,
                actions=torch.stack(acts, dim=1) if K else torch.zeros((B, 0, A), dtype=DT), relu_min=relu_min,
                clamped=n_clamped / max(1, B * K * A))


def leaves_of(inp, requires_grad=True, noise=True):
    """The differentiable inputs of a case as float64 torch leaves -> dict(st=[...], W=[...], b=[...], noise or None)"""
    t = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=DT, requires_grad=requires_grad)
    return dict(st=[t(v) for v in inp["st"]], W=[t(v) for v in inp["W"]], b=[t(v) for v in inp["b"]],
                noise=t(inp["noise"]) if (noise and inp.get("noise") is not None) else None)


def twin_run(env_name, spec, solver, inp, activation, K, sub, clip=CLIP, control=None, noise=True, reset=None, reset_rows=None):
    """-> (twin, leaves, outputs of policy_loop) with the graph alive"""
    twin = Twin(env_name, spec, solver, "step")
    lv = leaves_of(inp, noise=noise)
    out = policy_loop(twin, lv["st"], lv["W"], lv["b"], activation, lv["noise"], K, sub, clip, spec["tau"], refs=inp.get("refs"),
                      control=control, reset=reset, reset_rows=reset_rows)
    return twin, lv, out


def loss_of(out, group):
    """<cotangents, outputs> for one cotangent group: dict with any of obs, states, last, actions"""
    loss = torch.zeros((), dtype=DT)
    t = lambda v: torch.as_tensor(np.asarray(v, np.float64), dtype=DT)
    if group.get("obs") is not None:
        loss = loss + (out["obs"] * t(group["obs"])).sum()
    if group.get("states") is not None:
        loss = loss + sum((s * t(g)).sum() for s, g in zip(out["states"], group["states"]) if g is not None)
    if group.get("last") is not None:
        loss = loss + sum((s * t(g)).sum() for s, g in zip(out["last"], group["last"]) if g is not None)
    if group.get("actions") is not None and out["actions"].shape[1] > 0:
        loss = loss + (out["actions"] * t(group["actions"])).sum()
    return loss


def flat_params(W, b):
    """The layout of MLPPolicy.params: W_1, b_1, .., W_L, b_L, each row-major"""
    return np.concatenate([np.asarray(t, np.float64).reshape(-1) for pair in zip(W, b) for t in pair])


def twin_grads(lv, out, groups):
    """Gradients for several cotangent groups over one forward graph -> list of dict(state0=[S x [B]], noise [B, K, A] (None without
    noise), params flat) in float64 numpy; zeros where the loss does not reach an input."""
    S, L = len(lv["st"]), len(lv["W"])
    wrt = list(lv["st"]) + list(lv["W"]) + list(lv["b"]) + ([lv["noise"]] if lv["noise"] is not None else [])
    res = []
    for group in groups:
        loss = loss_of(out, group)
        gr = [None] * len(wrt) if loss.grad_fn is None else torch.autograd.grad(loss, wrt, allow_unused=True, retain_graph=True)
        z = [np.zeros(tuple(w.shape)) if g is None else g.numpy() for g, w in zip(gr, wrt)]
        res.append(dict(state0=z[:S], params=flat_params(z[S:S + L], z[S + L:S + 2 * L]),
                        noise=z[S + 2 * L] if lv["noise"] is not None else None))
    return res


def cotangent_groups(rng, B, rows, OW, S, K, A):
    """The four groups of the GPU test: all; grad_last_state alone; grad_obs alone; grad_actions alone (its grad_state0 exists only
    through the transposed network)"""
    g_obs = rng.normal(size=(B, rows, OW))
    g_states = [rng.normal(size=(B, rows)) for _ in range(S)]
    g_last = [rng.normal(size=B) for _ in range(S)]
    g_act = rng.normal(size=(B, K, A))
    return [dict(obs=g_obs, states=g_states, last=g_last, actions=g_act), dict(last=g_last), dict(obs=g_obs), dict(actions=g_act)]


GROUP_NAMES = ("all", "last_state", "obs", "actions")


def keep_mask(twin, out, activation, margin=KINK_MARGIN, relu_margin=RELU_MARGIN):
    """[B] bool: the environments outside every margin (model kinks and clamp bounds; ReLU pre-activations)"""
    kd = twin.kink_distance()
    keep = np.ones(out["relu_min"].shape[0], bool) if kd is None else kd.numpy() >= margin
    if activation == "relu":
        keep &= out["relu_min"].numpy() >= relu_margin
    return keep


@functools.lru_cache(maxsize=None)
def main_twin(env_name, deadtime, solver, net, activation):
    """The twin's rollout of a main case (helpers_policy.main_case), once per process -> (spec, inp, twin, leaves, out)"""
    spec, inp = hp.main_case(env_name, deadtime, net)
    twin, lv, out = twin_run(env_name, spec, solver, inp, activation, K_MAIN, substeps_of(env_name))
    return spec, inp, twin, lv, out
