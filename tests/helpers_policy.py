"""Inputs and references of the policy-rollout tests (tests/test_policy_host.py, tests/test_gpu_policy.py, tests/test_gpu_guard_policy.py):
seeded states, network parameters and exploration rows for every case, a numpy restatement of the MLP policy of
`vmap_sim_ahead_policy` (include/excenv.h excenv_policy_t) in float64 and, with an exact fused multiply-add, in the working dtype, that
policy looped over `oracle.step`, and the forward rounding bound of the policy."""
import functools

import numpy as np

import oracle
from helpers_feedback import B_MAIN, K_MAIN, CLIP, U, obs_width, substeps_of  # noqa: F401  (the shapes of the closed-loop tests)
from helpers_vjp import CASES, SOLVERS, case_spec, vjp_inputs  # noqa: F401  (CASES / SOLVERS: what the tests parametrise over)

# hidden widths: N1 no blocking divides; N2 both limits (width 64, four layers); N0 no hidden layer; N3 a single-unit hidden layer
NETS = {"N1": (11, 5), "N2": (64, 64, 3), "N0": (), "N3": (1,)}
ACTIVATIONS = ("relu", "tanh")
SEED = 91


def action_dim(env_name):
    return oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][1]


def policy_inputs(env_name, spec, hidden, B=B_MAIN, K=K_MAIN, control=None, seed=SEED):
    """Seeded inputs of one case, float64: dict(st, W, b, noise, refs, widths). States are helpers_vjp.vjp_inputs' (seed 91); then
    from default_rng(7091), in this order: all W_l ~ N(0, 1 / sqrt(d_{l-1})), all b_l ~ U(-0.1, 0.1), noise ~ U(-1.25, 1.25)
    [B, K, A]; last the references of the controlled fields inside the normalisation box. seed: another draw of the same
    distributions (the randomised tests, the second parameter set of the in-place update)."""
    A = action_dim(env_name)
    widths = (obs_width(env_name, control),) + tuple(hidden) + (A,)
    st, _ = vjp_inputs(env_name, spec, B, max(K, 1), seed)
    rng = np.random.default_rng(7000 + seed)
    W = [rng.normal(0.0, 1.0 / np.sqrt(n), (d, n)) for n, d in zip(widths[:-1], widths[1:])]
    b = [rng.uniform(-0.1, 0.1, d) for d in widths[1:]]
    noise = rng.uniform(-1.25, 1.25, (B, K, A))
    refs = None
    if control:
        refs = {}
        for name in control:
            lo, hi = spec["phys_norm"][name]
            refs[name] = (rng.uniform(-0.8, 0.8, B) + 1) / 2 * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) + np.asarray(lo, np.float64)
    return dict(st=st, W=W, b=b, noise=noise, refs=refs, widths=widths)


# ---- an exact fused multiply-add on the CPU, vectorised ----------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker's product with Veltkamp's split; no overflow / underflow at the magnitudes used here)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_odd_sum(a, b):
    """a + b rounded to odd in float64: the nearest-even sum, moved to its odd neighbour on the side of the error where it is inexact
    and even"""
    s, err = _two_sum(a, b)
    bits = s.view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    return np.where((err != 0) & even, np.nextafter(s, toward), s)


def fma_exact(a, b, c, dtype):
    """fma(a, b, c) with ONE rounding to `dtype`, elementwise, for finite operands held in `dtype`. float32: the product is exact in
    float64 and the sum is rounded to odd there before the final rounding (53 >= 2 * 24 + 2). float64: Boldo and Melquiond's
    emulation ("Emulation of a FMA and correctly rounded sums", 2008): error-free product and sums, the two low parts added with
    rounding to odd. tests/test_policy_host.py holds both against fractions.Fraction."""
    dtype = np.dtype(dtype)
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    a, b, c = a.copy(), b.copy(), c.copy()
    if dtype == np.float32:
        return _round_odd_sum(a * b, c).astype(np.float32)
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _round_odd_sum(tl, vl)


# ---- the policy --------------------------------------------------------------------------------------------------------------------
def mlp_np(ob, W, b, activation, noise_k, clip, exact=None):
    """The policy on one observation row in the contract's operation order: ob [B, OW], W / b the layers, noise_k [B, A] or None ->
    (a [B, A], raw [B, A] before the clamp, [hidden pre-activations [B, d_l]]). exact=None: float64 numpy with unfused
    multiply-adds (the independent reference). exact=np.float32 / np.float64: every operation as the kernel rounds it — fma_exact in
    that dtype, ReLU only (a tanh is not reproducible bit for bit)."""
    work = np.float64 if exact is None else np.dtype(exact).type
    x = np.asarray(ob, work)
    pre = []
    L = len(W)
    for l in range(L):
        Wl, bl = np.asarray(W[l], work), np.asarray(b[l], work)
        acc = np.broadcast_to(bl, (x.shape[0], bl.shape[0])).copy()
        for i in range(Wl.shape[1]):
            if exact is None:
                acc = Wl[None, :, i] * x[:, i:i + 1] + acc
            else:
                acc = fma_exact(Wl[None, :, i], x[:, i:i + 1], acc, work)
        if l < L - 1:
            pre.append(acc)
            if activation == "tanh":
                assert exact is None, "tanh has no bit-exact restatement"
                x = np.tanh(acc)
            else:
                x = np.where(acc < 0, work(0), acc)
        else:
            x = acc
    raw = x if noise_k is None else np.asarray(noise_k, work) + x
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    a = np.where(raw < work(lo), work(lo), raw)
    a = np.where(a > work(hi), work(hi), a)
    return a, raw, pre


def oracle_policy_loop(env_name, solver, props, inp, tau, activation, K=K_MAIN, sub=None, clip=CLIP, control=None, noise=True):
    """The float64 numpy policy looped over oracle.step ("step" semantics, solver step tau) -> dict(obs [B, N+1, OW], states
    (S x [B, N+1]), last, actions [B, K, A], clamped: the share of action entries the clamp changed, negative: the share of hidden
    pre-activations below zero (nan without a hidden layer))"""
    sub = substeps_of(env_name) if sub is None else sub
    st = [np.asarray(v, np.float64) for v in inp["st"]]
    B = st[0].shape[0]
    A = action_dim(env_name)
    ctl = [(n, inp["refs"][n]) for n in control] if control else None
    ob = oracle.sim_ahead(env_name, solver, st, np.zeros((B, 0, A)), props, tau, control=ctl)[0][:, 0]
    rows_o, rows_s, acts = [ob], [st], []
    n_clamped = n_neg = n_pre = 0
    for k in range(K):
        a, raw, pre = mlp_np(ob, inp["W"], inp["b"], activation, inp["noise"][:, k] if noise else None, clip)
        n_clamped += int(np.sum(a != raw))
        n_neg += sum(int(np.sum(p < 0)) for p in pre)
        n_pre += sum(p.size for p in pre)
        acts.append(a)
        for _ in range(sub):
            ob, st = oracle.step(env_name, solver, st, a, props, tau, control=ctl)
            rows_o.append(ob)
            rows_s.append(st)
    S = len(st)
    return dict(obs=np.stack(rows_o, axis=1), states=[np.stack([r[j] for r in rows_s], axis=1) for j in range(S)], last=st,
                actions=np.stack(acts, axis=1) if K else np.zeros((B, 0, A)), clamped=n_clamped / max(1, B * K * A),
                negative=n_neg / n_pre if n_pre else float("nan"))


def policy_bounds(obs_rows, W, b, activation, noise, clip, dtype):
    """From the observation rows of the action rows ([B, K, OW], as the kernel returned them) and the parameters and noise as the
    kernel saw them: the float64 actions [B, K, A] and the allowed distance of every entry, the forward bound of the contract's
    arithmetic. Per layer, with n = d_{l-1}, e the bound carried in (0 at the observations) and c = 2 (n + 4) u:
        m_j = |b_j| + sum_i |W_ji| (|x_i| + e_i);   e'_j = sum_i |W_ji| e_i + c m_j;   after tanh e'_j += 10 u |tanh y_j|
    (tanh and ReLU are 1-Lipschitz), at the end e_a = e_y + 2 u (|noise| + |y| + e_y); the clamp is 1-Lipschitz."""
    obs_rows = np.asarray(obs_rows, np.float64)
    B, K, OW = obs_rows.shape
    u = U[np.dtype(dtype)]
    x = obs_rows.reshape(B * K, OW)
    e = np.zeros_like(x)
    L = len(W)
    for l in range(L):
        Wl, bl = np.asarray(W[l], np.float64), np.asarray(b[l], np.float64)
        c = 2.0 * (Wl.shape[1] + 4) * u
        y = bl
        for i in range(Wl.shape[1]):
            y = Wl[None, :, i] * x[:, i:i + 1] + y
        m = np.abs(bl) + (np.abs(x) + e) @ np.abs(Wl).T
        e = e @ np.abs(Wl).T + c * m
        if l < L - 1:
            if activation == "tanh":
                x = np.tanh(y)
                e = e + 10.0 * u * np.abs(x)
            else:
                x = np.where(y < 0, 0.0, y)
        else:
            x = y
    A = x.shape[1]
    y = x.reshape(B, K, A)
    e = e.reshape(B, K, A)
    nz = np.zeros_like(y) if noise is None else np.asarray(noise, np.float64)
    raw = nz + y
    bound = e + (2.0 * u * (np.abs(nz) + np.abs(y) + e) if noise is not None else 0.0)
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    return np.minimum(np.maximum(raw, lo), hi), bound


# ---- the cases of the CPU suite's input condition and of the GPU suite --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_case(env_name, deadtime, net):
    """(spec, inputs) of a main case, float64, computed once per process"""
    spec = case_spec(env_name, deadtime)
    return spec, policy_inputs(env_name, spec, NETS[net])


@functools.lru_cache(maxsize=None)
def oracle_case(env_name, deadtime, solver, net, activation):
    """The independent fp64 closed loop of a main case, once per process (shared by the CPU input condition and GPU test 3)"""
    spec, inp = main_case(env_name, deadtime, net)
    B = inp["st"][0].shape[0]
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    return oracle_policy_loop(env_name, solver, props, inp, spec["tau"], activation)
