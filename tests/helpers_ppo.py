"""Inputs and references of the tests of excenv_gaussian_logp / excenv_ppo_loss / excenv_ppo_loss_grad and `vmap_gaussian_logp` /
`vmap_ppo_loss` (tests/test_ppo_host.py, tests/test_gpu_ppo_loss.py):
- the numpy twin of the contract block of include/excenv.h, every operation rounded as the kernel rounds it (helpers_policy.fma_exact),
  with the likelihood ratio r taken as an argument (the device's exp is the one operation numpy cannot restate bit for bit);
- the same block in np.longdouble, the reference;
- seeded inputs with fixed pattern lanes, the conditions the tests check before a launch, and the rounding bounds."""
import functools
import math

import numpy as np

import helpers_policy as hp

B_SIZES = (1, 63, 64, 65, 326, 1028)
K_SIZES = (1, 2, 9)
A_SIZES = (1, 2)
MAX_GROUPS = (0, 1, 3)
DTYPES = ("float32", "float64")
CLIP_EPS = 0.2
N_STATS, TILE, AUTO_GROUPS, MAX_ACTION = 5, 1024, 2048, 2  # include/excenv.h
N_PATTERN = 4  # pattern lanes: reset[0], reset[K-1], a run of resets, every reset
# The shares of clipped / inactive samples are statistics: they are asserted where a case holds at least this many samples
MIN_SAMPLES = 500
EPS = {"float32": 2.0 ** -23, "float64": 2.0 ** -52}


def consts(log_std, dtype):
    """(inv_std [A], logp_const) as `vmap_ppo_loss` computes them: in float64, then rounded to `dtype` (held in float64)"""
    ls = np.asarray(log_std, np.float64)
    return np.exp(-ls).astype(dtype).astype(np.float64), float(np.asarray(-ls.sum() - 0.5 * len(ls) * math.log(2.0 * math.pi)).astype(dtype))


def clip_bounds(clip_eps, dtype):
    """lo = (T)(1 - clip_eps), hi = (T)(1 + clip_eps), folded in double"""
    return float(np.asarray(1.0 - clip_eps).astype(dtype)), float(np.asarray(1.0 + clip_eps).astype(dtype))


def groups_of(B, K, max_groups):
    """policy.hpp ppo_tiles / ppo_groups restated -> (tiles, workgroups)"""
    tiles = K * ((B + TILE - 1) // TILE)
    return tiles, min(tiles, max_groups if max_groups > 0 else AUTO_GROUPS)


def workspace_bytes(B, K, max_groups):
    return groups_of(B, K, max_groups)[1] * (N_STATS + MAX_ACTION) * 8


def first_tile(tiles, groups, g):
    return g * (tiles // groups) + min(g, tiles % groups)


def ppo_twin(mean, sample, inv_std, logp_const, logp_old=None, advantage=None, value=None, returns=None, reset=None, clip_eps=CLIP_EPS,
             adv_norm=None, grad_scale=(1.0, 1.0), dtype="float64", r=None, ref=False):
    """The contract block in numpy on arrays [B, K, A] / [B, K]. ref=False: in `dtype`, every rounding the kernel's (one rounding per
    operation, the multiply-adds of logp fused), r given (None: numpy's exp in `dtype`, for the input conditions only). ref=True: in
    np.longdouble from the same inputs, r = exp(d). logp_old None: only z and logp (excenv_gaussian_logp).
    -> dict(z, logp, d, r, a, s1, s2, surr, active, clipped, valid, terms {n, surr, vsq, kl, clip, gls [B, K, A]} (0 where invalid),
    grad_mean [B, K, A], grad_value [B, K])"""
    T = np.longdouble if ref else np.dtype(dtype).type
    arr = lambda x: np.asarray(x, np.float64).astype(T)
    fma = (lambda a, b, c: a * b + c) if ref else (lambda a, b, c: hp.fma_exact(a, b, c, T).astype(T))
    m, x, istd = arr(mean), arr(sample), arr(inv_std)
    B, K, A = m.shape
    out = {}
    with np.errstate(all="ignore"):
        z = ((x - m) * istd[None, None, :]).astype(T)
        lp = np.full((B, K), T(logp_const), T)
        for q in range(A):
            lp = fma((T(-0.5) * z[..., q]).astype(T), z[..., q], lp)
        out.update(z=z, logp=lp)
        if logp_old is None:
            return out
        lo, hi = (T(v) for v in clip_bounds(clip_eps, dtype))
        d = (lp - arr(logp_old)).astype(T)
        if ref:
            r = np.exp(d)
        elif r is None:
            r = np.exp(d).astype(T)
        r = np.asarray(r, T)
        a = arr(advantage)
        if adv_norm is not None:
            a = ((a - T(np.asarray(adv_norm[0]).astype(dtype))) * T(np.asarray(adv_norm[1]).astype(dtype))).astype(T)
        s1 = (r * a).astype(T)
        rl = np.where(r < lo, lo, r)
        rc = np.where(rl > hi, hi, rl).astype(T)
        s2 = (rc * a).astype(T)
        active = ~(s2 < s1)
        surr = np.where(s2 < s1, s2, s1)
        clipped = (r < lo) | (r > hi)
        valid = np.ones((B, K), bool) if reset is None else ~np.asarray(reset, bool)
        dv = (arr(value) - arr(returns)).astype(T) if value is not None else np.zeros((B, K), T)
        g0 = np.where(active, -s1, T(0))
        zero = T(0)
        gls = np.stack([np.where(valid, (g0 * ((z[..., q] * z[..., q]).astype(T) - T(1)).astype(T)).astype(T), zero) for q in range(A)], -1)
        terms = dict(n=valid.astype(np.float64), surr=np.where(valid, surr, zero), vsq=np.where(valid, (dv * dv).astype(T), zero),
                     kl=np.where(valid, ((r - T(1)).astype(T) - d).astype(T), zero), clip=(valid & clipped).astype(np.float64), gls=gls)
        w, wv = (T(np.asarray(v).astype(dtype)) for v in grad_scale)
        gl = np.where(active, ((-s1) * w).astype(T), zero)
        gm = np.stack([np.where(valid, ((gl * z[..., q]).astype(T) * istd[q]).astype(T), zero) for q in range(A)], -1)
        gv = np.where(valid, (wv * dv).astype(T), zero)
    out.update(d=d, r=r, a=a, s1=s1, s2=s2, surr=surr, active=active, clipped=clipped, valid=valid, terms=terms, grad_mean=gm, grad_value=gv)
    return out


def stat_terms(terms, A):
    """The terms of the EXCENV_PPO_STATS + A sums, in the order of `stats`: list of [B, K] float64 arrays"""
    return [np.asarray(terms[k], np.float64) for k in ("n", "surr", "vsq", "kl", "clip")] + [np.asarray(terms["gls"][..., q], np.float64) for q in range(A)]


def pattern_reset(K):
    """[N_PATTERN, K] bool: reset[0]; reset[K-1]; a run of resets in the middle (rows K//3 .. 2K//3); every row"""
    cut = np.zeros((N_PATTERN, K), bool)
    cut[0, 0] = True
    cut[1, K - 1] = True
    cut[2, K // 3:2 * K // 3 + 1] = True
    cut[3, :] = True
    return cut


@functools.lru_cache(maxsize=None)
def ppo_case(B, K, A, dtype="float64", seed=0):
    """Seeded inputs rounded to `dtype`, held as float64: log_std [A] ~ U(-1.2, -0.3); mean_old [B, K, A] ~ N(0, 0.5); sample = mean_old
    + exp(log_std) N(0, 1); advantage, value, returns [B, K] ~ N(0, 1); reset [B, K] with P drawn from U(0.1, 0.3), the first
    N_PATTERN lanes pattern_reset where B > N_PATTERN; mean = mean_old + 0.15 exp(log_std) / sqrt(A) N(0, 1), the changed policy.
    Shared: do not modify."""
    rng = np.random.default_rng([1900, B, K, A, seed])
    rd = lambda v: np.asarray(v).astype(dtype).astype(np.float64)
    log_std = rng.uniform(-1.2, -0.3, A)
    std = np.exp(log_std)
    mean_old = rd(rng.normal(0.0, 0.5, (B, K, A)))
    sample = rd(mean_old + std * rng.normal(size=(B, K, A)))
    adv, val, ret = (rd(rng.normal(size=(B, K))) for _ in range(3))
    reset = rng.random((B, K)) < rng.uniform(0.1, 0.3)
    n_fixed = N_PATTERN if B > N_PATTERN else 0
    reset[:n_fixed] = pattern_reset(K)[:n_fixed]
    mean = rd(mean_old + 0.15 * std / np.sqrt(A) * rng.normal(size=(B, K, A)))
    return dict(B=B, K=K, A=A, dtype=dtype, log_std=log_std, mean_old=mean_old, sample=sample, advantage=adv, value=val, returns=ret,
                reset=reset, mean=mean, n_fixed=n_fixed)


def changed(case, inv_std=None, logp_const=None, **kw):
    """(twin in the case's dtype, long-double reference) of the changed policy; both carry logp_old [B, K], the twin's logp of mean_old"""
    if inv_std is None:
        inv_std, logp_const = consts(case["log_std"], case["dtype"])
    old = ppo_twin(case["mean_old"], case["sample"], inv_std, logp_const, dtype=case["dtype"])["logp"]
    args = dict(logp_old=old, advantage=case["advantage"], value=case["value"], returns=case["returns"], reset=case["reset"], dtype=case["dtype"])
    args.update(kw)
    twin = ppo_twin(case["mean"], case["sample"], inv_std, logp_const, **args)
    ref = ppo_twin(case["mean"], case["sample"], inv_std, logp_const, ref=True, **args)
    twin["logp_old"] = ref["logp_old"] = np.asarray(old, np.float64)
    return twin, ref


def input_conditions(twin, ref):
    """(share of clipped ratios, share of inactive samples, share of samples whose active bit or clip indicator differs between the
    twin and the reference, number of valid samples), over the valid samples"""
    v = twin["valid"]
    n = int(v.sum())
    if n == 0:
        return 0.0, 0.0, 0.0, 0
    flips = (twin["active"] != ref["active"]) | (twin["clipped"] != ref["clipped"])
    return float(ref["clipped"][v].mean()), float((~ref["active"])[v].mean()), float(flips[v].mean()), n


def rel_bound(case_dtype, A, logp_const, logp, logp_old):
    """eps_T (8 + 2 (A + 2) (|logp_const| + |logp| + |logp_old|)), [B, K]: the relative bound of -(r a) w z inv_std against the exact
    value. d = logp - logp_old carries the A + 1 roundings of logp (each at most eps/2 of a partial sum no larger than |logp_const| +
    |logp|) and the subtraction's (eps/2 |d|): |delta d| <= eps/2 (A + 2)(|logp_const| + |logp| + |logp_old|); r = exp(d) turns it into
    a relative error, doubled for the 2-ulp exp with room to spare; the four products, the subtraction in z and the rounded inv_std
    add at most 8 eps/2 ... 8 eps."""
    e = EPS[case_dtype]
    return e * (8.0 + 2.0 * (A + 2) * (abs(float(logp_const)) + np.abs(np.asarray(logp, np.float64)) + np.abs(np.asarray(logp_old, np.float64))))


def term_bounds(ref, rel, dtype, A):
    """Absolute bounds of the terms of the sums, in the order of `stats`, against the long-double terms (0 where invalid), from `rel`
    (rel_bound): n and S_clip are counts; surr is a product like the gradient (rel |surr|); (value - returns)^2 has three roundings (4
    eps); the KL term (r - 1) - d cancels, so its error is absolute: |delta r| + |delta d| + eps (|r - 1| + |term|) with |delta r| <=
    rel r and |delta d| <= rel; z^2 - 1 cancels too: |g0| eps (3 z^2 + 1) + rel |term|."""
    e = EPS[dtype]
    f = lambda x: np.abs(np.asarray(x, np.float64))
    t = ref["terms"]
    v = ref["valid"]
    zero = np.zeros_like(rel)
    r, d = f(ref["r"]), f(ref["d"])
    kl = np.where(v, rel * r + rel + e * (f(ref["r"] - 1) + f(t["kl"])), 0.0)
    g0 = np.where(ref["active"], f(ref["s1"]), 0.0)
    gls = [np.where(v, g0 * e * (3.0 * f(ref["z"][..., q]) ** 2 + 1.0) + rel * f(t["gls"][..., q]), 0.0) for q in range(A)]
    return [zero, rel * f(t["surr"]), 4.0 * e * f(t["vsq"]), kl, zero] + gls


def same_bits(a, b):
    """Equal bits, a NaN standing for any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    word = np.int32 if a.dtype == np.float32 else np.int64
    return bool(np.all((a.view(word) == b.view(word)) | (np.isnan(a) & np.isnan(b))))
