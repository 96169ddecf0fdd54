"""Inputs and the float64 restatement for the tests of the policy's parameter gradient (excenv_policy_param_grad, `vmap_policy_param_grads`;
tests/test_policy_param_grad_host.py, tests/test_gpu_policy_param_grad.py, tests/test_gpu_guard_policy_param_grad.py):
- the restatement on the CPU: torch.autograd.grad(helpers_policy_vjp.torch_mlp(rows64), params64, g64) on given arrays;
- seeded random observation rows / grad_raw rows / parameters for a width tuple; for ReLU the rows are redrawn until no hidden
  pre-activation lies within RELU_MARGIN_FP64 of 0 (checked here on the CPU: `relu_min`);
- the sample tiles and the workgroups' tile ranges of include/excenv.h, restated."""
import functools

import numpy as np
import torch

import helpers_policy as hp
import helpers_policy_vjp as hv
from helpers_policy_vjp import RELU_MARGIN_FP64  # noqa: F401

TILE = 64
AUTO_GROUPS = 512
# the hidden layers of the entry's own test: helpers_policy.NETS, both limits three times over, every tile full
NETS = dict(hp.NETS, W3=(64, 64, 64), F3=(16, 16, 16))


def param_count(widths):
    return sum(d * (n + 1) for n, d in zip(widths[:-1], widths[1:]))


def restatement(W, b, activation, rows, g):
    """rows [n, OW], g [n, A], float64 -> the flat gradient of sum(g * mlp(rows)) in the layout of MLPPolicy.params"""
    t = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=torch.float64, requires_grad=True)
    Wt, bt = [t(w) for w in W], [t(v) for v in b]
    y = hv.torch_mlp(torch.as_tensor(np.asarray(rows, np.float64)), Wt, bt, activation)
    gr = torch.autograd.grad(y, Wt + bt, torch.as_tensor(np.asarray(g, np.float64)))
    L = len(W)
    return hv.flat_params([x.numpy() for x in gr[:L]], [x.numpy() for x in gr[L:]])


def term_magnitudes(W, b, activation, rows, g):
    """The flat sum over the samples of |the sample's own term| of every parameter's gradient, float64: sum_n |d^l_n[j]| |x^{l-1}_n[i]|
    for W_l[j][i] and sum_n |d^l_n[j]| for b_l[j] (plain backpropagation in numpy)"""
    xs = [np.asarray(rows, np.float64)]
    L = len(W)
    for l in range(L - 1):
        y = xs[-1] @ np.asarray(W[l]).T + np.asarray(b[l])
        xs.append(np.tanh(y) if activation == "tanh" else np.maximum(y, 0.0))
    d = np.asarray(g, np.float64)
    mw, mb = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        mw[l], mb[l] = np.abs(d).T @ np.abs(xs[l]), np.abs(d).sum(axis=0)
        if l > 0:
            back = d @ np.asarray(W[l])
            d = back * ((1.0 - xs[l] * xs[l]) if activation == "tanh" else (xs[l] > 0))
    return hv.flat_params(mw, mb)


def relu_min(W, b, rows):
    """[n]: the smallest absolute hidden pre-activation of every row (inf without a hidden layer)"""
    pre = []
    hv.torch_mlp(torch.as_tensor(np.asarray(rows, np.float64)), [torch.as_tensor(w) for w in W], [torch.as_tensor(v) for v in b], "relu", pre)
    if not pre:
        return np.full(len(rows), np.inf)
    return np.min(np.stack([p.abs().min(dim=1).values.numpy() for p in pre]), axis=0)


@functools.lru_cache(maxsize=None)
def random_case(widths, activation, B, K, sub=3, seed=0, dtype="float64"):
    """Seeded arrays for a width tuple, rounded to `dtype` and held as float64: dict(W, b, obs [B, K * sub + 1, OW], graw [B, K, A],
    rows [B * K, OW] and g [B * K, A] (the samples, k-major as the kernel's tiles), relu_min (smallest |pre-activation|, ReLU only)).
    Do not modify what this returns: it is shared."""
    rng = np.random.default_rng(4200 + seed)
    r = lambda v: np.asarray(v).astype(dtype).astype(np.float64)
    W = [r(rng.normal(0.0, 1.0 / np.sqrt(n), (d, n))) for n, d in zip(widths[:-1], widths[1:])]
    b = [r(rng.uniform(-0.1, 0.1, d)) for d in widths[1:]]
    obs = r(rng.uniform(-1.0, 1.0, (B, K * sub + 1, widths[0])))
    graw = r(rng.normal(size=(B, K, widths[-1])))
    low = np.inf
    if activation == "relu" and K > 0:
        for _ in range(50):
            rows = obs[:, 0:K * sub:sub].reshape(B * K, widths[0])
            m = relu_min(W, b, rows).reshape(B, K)
            bad = m < 2 * RELU_MARGIN_FP64
            low = float(m.min())
            if not bad.any():
                break
            bi, ki = np.nonzero(bad)
            obs[bi, ki * sub] = r(rng.uniform(-1.0, 1.0, (len(bi), widths[0])))
    rows = obs[:, 0:K * sub:sub].transpose(1, 0, 2).reshape(B * K, widths[0])
    g = graw.transpose(1, 0, 2).reshape(B * K, widths[-1])
    return dict(W=W, b=b, obs=obs, graw=graw, rows=rows, g=g, relu_min=low, widths=widths)


def _entry_cases():
    """(net, activation, OW, A, B, K) of the entry's own fp64 test: every network with both activations at the main shape, OW and A
    going round; N1 (no tile divides) and W3 (both limits) over every batch edge and both row counts; N1 ReLU over every OW x A"""
    acts = hp.ACTIVATIONS
    cases = [(net, act, (3, 8, 16)[i % 3], (1, 2)[(i // 2) % 2], hp.B_MAIN, hp.K_MAIN)
             for i, (net, act) in enumerate((n, a) for n in ("N1", "N2", "N0", "N3", "W3", "F3") for a in acts)]
    cases += [(net, "tanh", 8, 2, B, K) for net in ("N1", "W3") for B in (1, 63, 64, 65, hp.B_MAIN) for K in (1, hp.K_MAIN)]
    cases += [("N1", "relu", OW, A, 65, hp.K_MAIN) for OW in (3, 8, 16) for A in (1, 2)]
    return list(dict.fromkeys(cases))


ENTRY_CASES = _entry_cases()


def entry_case(net, activation, OW, A, B, K, dtype="float64"):
    return random_case((OW,) + tuple(NETS[net]) + (A,), activation, B, K, 3, 0, dtype)


# ---- the tiles and their workgroups (include/excenv.h) ---------------------------------------------------------------------------------
def tiles(B, K):
    return K * ((B + TILE - 1) // TILE)


def groups(B, K, max_groups=0):
    return min(tiles(B, K), max_groups if max_groups > 0 else AUTO_GROUPS)


def first_tile(T, G, g):
    return g * (T // G) + min(g, T % G)


def tile_ranges(B, K, max_groups=0):
    """[(first tile, one past the last tile)] per workgroup"""
    T, G = tiles(B, K), groups(B, K, max_groups)
    return [(first_tile(T, G, g), first_tile(T, G, g + 1)) for g in range(G)]


def workspace_bytes(B, K, widths, max_groups=0):
    return groups(B, K, max_groups) * param_count(widths) * 8


def lds_bytes(widths, elem):
    return (sum(widths) + 1) * (TILE + 2) * elem
