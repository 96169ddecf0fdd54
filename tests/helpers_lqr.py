"""The numpy twin of excenv_lqr_backward's contract block (include/excenv.h) and the seeded cases of the LQR tests
(tests/test_lqr_host.py, tests/test_gpu_lqr.py, tests/test_gpu_guard_lqr.py).

The twin runs in the working dtype, lane by lane in the same order as the header writes it: every `fma` of the block is
helpers_policy.fma_exact (one rounding), every other operation numpy's in that dtype, so a kernel that follows the block gives the same
bits. It is vectorised over the environments (the first axis), which never mix. It records the state after every row, so ONE run over N
rows also is the twin of the calls over the last 1, 2, .. rows of the same data: `twin.at(m)` is the call with N = m on rows N - m ..
N - 1 (time-invariant: m iterations)."""
import functools

import numpy as np

from helpers_policy import fma_exact

SHAPES = ((1, 1), (2, 1), (4, 1), (7, 2))
DTYPES = ("float32", "float64")
B_SIZES = (1, 63, 64, 65, 326)
N_SIZES = (0, 1, 2, 9)
B_MAX, N_MAX = max(B_SIZES), max(N_SIZES)


def bytes_per_row(dtype, S, A, time_invariant, has_q, has_r, store_all, has_ff):
    """excenv_lqr_backward_bytes restated"""
    elem = np.dtype(dtype).itemsize
    n = 0 if time_invariant else S * (S + A)
    n += S * bool(has_q) + A * bool(has_r)
    if store_all:
        n += A * S + A * bool(has_ff)
    return n * elem


class Twin:
    """What `lqr_twin` returns. gain [B, N, A, S], ff [B, N, A]: every row; P [N + 1][B, S, S], p [N + 1][B, S], dV [N + 1][B, 2],
    n_bad [N + 1][B]: entry m is the state after m rows from the end (entry 0: P = Qf, p = q[N])."""

    def __init__(self, N):
        self.N = N
        self.gain, self.ff, self.P, self.p, self.dV, self.n_bad = None, None, [], [], [], []

    def at(self, m, store_all=1):
        """The outputs of the call over the last m rows -> dict(gain [B, m or min(m, 1), A, S], ff, P0, p0, dV, n_bad)"""
        lo = self.N - m
        rows = slice(lo, self.N) if store_all else slice(lo, lo + min(m, 1))
        return dict(gain=self.gain[:, rows], ff=self.ff[:, rows], P0=self.P[m], p0=self.p[m], dV=self.dV[m], n_bad=self.n_bad[m])


def lqr_twin(F, G, Q, R, Qf=None, q=None, r=None, reg=0.0, dtype="float64", n_iter=None):
    """The contract block of excenv_lqr_backward. F [B, N, S, S], G [B, N, S, A] (time-invariant: [B, S, S], [B, S, A] with n_iter = N);
    Q, Qf [S, S], R [A, A]; q [B, N + 1, S], r [B, N, A] or None -> Twin"""
    t = np.dtype(dtype).type
    F, G = np.asarray(F, t), np.asarray(G, t)
    invariant = F.ndim == 3
    N = n_iter if invariant else F.shape[1]
    B, S, A = F.shape[0], F.shape[-1], G.shape[-1]
    Q, R = np.asarray(Q, t), np.asarray(R, t)
    Qf = Q if Qf is None else np.asarray(Qf, t)
    q = np.zeros((B, N + 1, S), t) if q is None else np.asarray(q, t)
    r = np.zeros((B, N, A), t) if r is None else np.asarray(r, t)
    reg = t(reg)

    def fma(a, b, c):
        """fma_exact, with the sign of an exact zero as IEEE 754 gives it: the emulation's error-free sums return +0 for (-0) + (-0).
        Where the exact result is zero, the product is exact and the plain a * b + c has that zero with the right sign."""
        a, b, c = np.asarray(a, t), np.asarray(b, t), np.asarray(c, t)
        exact, plain = fma_exact(a, b, c, t), a * b + c
        return np.where((exact == 0) & (plain == 0), plain, exact).astype(t)

    iu = np.triu_indices(S)
    sym = lambda M: np.triu(M) + np.triu(M, 1).T  # [i][j] = M[min][max]
    half = t(0.5)

    out = Twin(N)
    out.gain, out.ff = np.zeros((B, N, A, S), t), np.zeros((B, N, A), t)
    P = np.broadcast_to(sym(Qf), (B, S, S)).copy()
    p = q[:, N].copy()
    dV = np.zeros((B, 2), t)
    bad = np.zeros(B, np.int32)
    out.P.append(P.copy()), out.p.append(p.copy()), out.dV.append(dV.copy()), out.n_bad.append(bad.copy())
    with np.errstate(all="ignore"):
        for n in range(N - 1, -1, -1):
            Fn, Gn = (F, G) if invariant else (F[:, n], G[:, n])
            # W[i][j] = P[i][0] * F[0][j]; k >= 1: fma(P[i][k], F[k][j], .)   (likewise Wb with G)
            W = P[:, :, 0, None] * Fn[:, 0, None, :]
            Wb = P[:, :, 0, None] * Gn[:, 0, None, :]
            for k in range(1, S):
                W = fma(P[:, :, k, None], Fn[:, k, None, :], W)
                Wb = fma(P[:, :, k, None], Gn[:, k, None, :], Wb)
            # Qxx[i][j] = Q[i][j]; k: fma(F[k][i], W[k][j], .)    (used in the upper triangle only)
            Qxx = np.broadcast_to(Q, (B, S, S)).astype(t)
            Quu = np.broadcast_to(R, (B, A, A)).astype(t)
            Qx, Qu = q[:, n].copy(), r[:, n].copy()
            for k in range(S):
                Qxx = fma(Fn[:, k, :, None], W[:, k, None, :], Qxx)
                Quu = fma(Gn[:, k, :, None], Wb[:, k, None, :], Quu)
                Qx = fma(Fn[:, k, :], p[:, k, None], Qx)
                Qu = fma(Gn[:, k, :], p[:, k, None], Qu)
            Qux = Gn[:, 0, :, None] * W[:, 0, None, :]
            for k in range(1, S):
                Qux = fma(Gn[:, k, :, None], W[:, k, None, :], Qux)
            if A == 2:
                Quu[:, 1, 0] = Quu[:, 0, 1]
            # the solve: right-hand columns g = -Qux[.][j] and g = -Qu
            g = np.concatenate([-Qux, -Qu[:, :, None]], axis=2)  # [B, A, S + 1]
            d0 = Quu[:, 0, 0] + reg
            if A == 1:
                ok = d0 > 0
                x = g / d0[:, None, None]
            else:
                l = Quu[:, 0, 1] / d0
                d1 = fma(-l, Quu[:, 0, 1], Quu[:, 1, 1] + reg)
                ok = (d0 > 0) & (d1 > 0)
                y1 = fma(-l[:, None], g[:, 0], g[:, 1])
                x1 = y1 / d1[:, None]
                x0 = fma(-l[:, None], x1, g[:, 0] / d0[:, None])
                x = np.stack([x0, x1], axis=1)
            x = np.where(ok[:, None, None], x, t(0)).astype(t)
            bad = bad + (~ok).astype(np.int32)
            K, kf = x[:, :, :S], x[:, :, S]
            QK = Quu[:, :, 0, None] * K[:, 0, None, :]
            Qk = Quu[:, :, 0] * kf[:, 0, None]
            for c in range(1, A):
                QK = fma(Quu[:, :, c, None], K[:, c, None, :], QK)
                Qk = fma(Quu[:, :, c], kf[:, c, None], Qk)
            Pn, pn = Qxx, Qx
            for a in range(A):
                Pn = fma(K[:, a, :, None], QK[:, a, None, :], Pn)
                pn = fma(K[:, a, :], Qk[:, a, None], pn)
            for a in range(A):
                Pn = fma(K[:, a, :, None], Qux[:, a, None, :], Pn)
                pn = fma(K[:, a, :], Qu[:, a, None], pn)
            for a in range(A):
                Pn = fma(Qux[:, a, :, None], K[:, a, None, :], Pn)
                pn = fma(Qux[:, a, :], kf[:, a, None], pn)
            P = np.zeros((B, S, S), t)
            P[:, iu[0], iu[1]] = Pn[:, iu[0], iu[1]]
            P[:, iu[1], iu[0]] = Pn[:, iu[0], iu[1]]
            p = pn
            h = kf[:, 0] * Qk[:, 0]
            for a in range(1, A):
                h = fma(kf[:, a], Qk[:, a], h)
            dV = dV.copy()
            for a in range(A):
                dV[:, 0] = fma(kf[:, a], Qu[:, a], dV[:, 0])
            dV[:, 1] = dV[:, 1] + half * h
            out.gain[:, n], out.ff[:, n] = K, kf
            out.P.append(P.copy()), out.p.append(p.copy()), out.dV.append(dV.copy()), out.n_bad.append(bad.copy())
    return out


def same_bits(a, b):
    """Equal bit for bit, a NaN standing for any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | nan))


# ---------------------------------------------------------------------------------------------------------------- the seeded cases
def random_problem(S, A, B, N, seed=0, rho=0.95):
    """Stable-ish random LQR data in float64: F_n = rho-scaled random matrices near a rotation-free contraction (spectral norm about
    rho), G_n ~ N(0, 1) / sqrt(S), Q = M M^T / S + 0.1 I, Qf likewise, R = M M^T / A + 0.5 I, q, r ~ U(-1, 1)."""
    rng = np.random.default_rng(1000 * S + 10 * A + seed)
    F = rng.normal(0.0, 1.0, (B, N, S, S))
    F = rho * F / np.maximum(np.linalg.norm(F, 2, axis=(-2, -1))[..., None, None], 1e-3)
    G = rng.normal(0.0, 1.0, (B, N, S, A)) / np.sqrt(S)

    def spd(n, shift):
        M = rng.normal(0.0, 1.0, (n, n))
        return M @ M.T / n + shift * np.eye(n)

    return dict(F=F, G=G, Q=spd(S, 0.1), Qf=spd(S, 0.1), R=spd(A, 0.5), q=rng.uniform(-1, 1, (B, N + 1, S)), r=rng.uniform(-1, 1, (B, N, A)))


def rounded(case, dtype):
    """The case with every array rounded to the working dtype: what both the kernel and the twin are given"""
    t = np.dtype(dtype).type
    return {k: np.asarray(v, t) for k, v in case.items()}


@functools.lru_cache(maxsize=None)
def grid_case(S, A, dtype):
    """The data of the GPU grid for one shape and type: B_MAX lanes, N_MAX rows (smaller calls are prefixes of the lanes and the last
    rows), rounded to the working dtype"""
    return rounded(random_problem(S, A, B_MAX, N_MAX, seed=3), dtype)


@functools.lru_cache(maxsize=None)
def grid_twin(S, A, dtype, with_lin, reg, invariant):
    """The twin of the grid case; invariant: row N_MAX - 1 of the Jacobians for every row"""
    c = grid_case(S, A, dtype)
    kw = dict(Qf=c["Qf"], q=c["q"] if with_lin else None, r=c["r"] if with_lin else None, reg=reg, dtype=dtype)
    if invariant:
        return lqr_twin(c["F"][:, -1], c["G"][:, -1], c["Q"], c["R"], n_iter=N_MAX, **kw)
    return lqr_twin(c["F"], c["G"], c["Q"], c["R"], **kw)


# ---------------------------------------------------------------------------------------------------------------- the C entry
def raw_lqr(dtype, B, N, S, A, jac, stride, Q, Qf, R, q, r, reg, store_all, gain, ff, P0, p0, dV, n_bad, expect=0):
    """excenv_lqr_backward straight through ctypes on device addresses (None: NULL), on the current stream of the current device"""
    import ctypes

    import torch

    from exciting_environments_amd import _native

    lib = _native.lib()
    rec = _native.Lqr(S, A, jac, stride, Q, Qf, R, q, r, float(reg), store_all, gain, ff, P0, p0, dV, n_bad)
    stream = _native._raw_stream(torch.device("cuda", torch.cuda.current_device()))
    rc = lib.excenv_lqr_backward(_native.dtype_id(dtype), B, N, ctypes.byref(rec), stream)
    assert rc == expect, lib.excenv_last_error()
    if B > 0 and rc == 0:
        assert _native.last_launch() == "riccati_kernel"


# ---------------------------------------------------------------------------------------------------------------- end to end on cart-pole
# Regulation at the upright equilibrium (theta = 0, every other state 0, zero force), Euler steps of 20 ms. Chosen on the CPU oracle
# (cartpole_reference; tests/test_lqr_host.py asserts the conditions on it): perturbations of at most E2E_PERTURB of each field's
# normalisation span around the equilibrium, E2E_ITERS Riccati iterations for the stationary gain, E2E_STEPS closed-loop steps.
E2E_TAU = 0.02
E2E_B = 64
E2E_PERTURB = 0.01
E2E_ITERS = 400
E2E_STEPS = 250
E2E_Q = np.diag([1.0, 0.1, 10.0, 0.1])
E2E_R = np.array([[10.0]])


def cartpole_spec():
    from helpers import spec_of

    spec = spec_of("cartpole")
    spec["tau"] = E2E_TAU
    return spec


def cartpole_start(B=E2E_B, seed=4):
    """Seeded physical states around the upright equilibrium: every field within E2E_PERTURB of its normalisation span -> S x [B]"""
    spec = cartpole_spec()
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, B) * E2E_PERTURB * (spec["phys_norm"][n][1] - spec["phys_norm"][n][0])
            for n in ("deflection", "velocity", "theta", "omega")]


def feedback_np(K, x_ref, u_ref, lo, hi, OW):
    """`lqr_feedback` in float64 numpy: K [B, A, S] -> (gain [B, A, OW], ff [B, A])"""
    B, A, S = K.shape
    half = (hi - lo) / 2
    gain = np.zeros((B, A, OW))
    gain[:, :, :S] = K * half
    return gain, u_ref + (K * np.broadcast_to((lo + half) - x_ref, (B, S))[:, None, :]).sum(axis=-1)


@functools.lru_cache(maxsize=None)
def cartpole_reference():
    """The whole chain on the CPU oracle in float64: central differences of oracle.step at the equilibrium for (F, G) (the velocity column beside the friction kink), the twin's
    stationary gain, the observation feedback, E2E_STEPS closed-loop Euler steps and the same steps with zero gain ->
    dict(K [1, 4], start S x [B], dist0 [B], dist_closed [B], dist_open [B], max_action)"""
    import oracle

    spec = cartpole_spec()
    names = ("deflection", "velocity", "theta", "omega")
    S = 4
    props, keep = oracle.make_props("cartpole", spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, 2 * (S + 1))
    h = 1e-6
    st = [np.zeros(2 * (S + 1)) for _ in range(S)]
    act = np.zeros((2 * (S + 1), 1))
    for j in range(S):
        st[j][2 * j], st[j][2 * j + 1] = h, -h
    # the Coulomb friction of the cart has a kink at velocity 0, whose derivative the kernels take as 0: that column is differenced
    # beside the kink
    st[1][2:4] += 1e-3
    act[2 * S, 0], act[2 * S + 1, 0] = h, -h
    new = np.stack(oracle.step("cartpole", "euler", st, act, props, E2E_TAU)[1], axis=0)  # [S, 2 (S + 1)]
    J = (new[:, 0::2] - new[:, 1::2]) / (2 * h)  # [S, S + 1]
    F, G = J[None, :, :S], J[None, :, S:]
    K = lqr_twin(F, G, E2E_Q, E2E_R, n_iter=E2E_ITERS).at(E2E_ITERS, store_all=0)["gain"][:, 0]  # [1, 1, 4]
    lo = np.array([spec["phys_norm"][n][0] for n in names], np.float64)
    hi = np.array([spec["phys_norm"][n][1] for n in names], np.float64)
    start = cartpole_start()
    B = start[0].shape[0]
    gain, ff = feedback_np(np.broadcast_to(K, (B, 1, S)), np.zeros(S), np.zeros(1), lo, hi, S)
    props, keep2 = oracle.make_props("cartpole", spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    out = dict(K=K[0], start=start, F=F[0], G=G[0])
    dist = lambda s: np.sqrt(sum(v * v for v in s))
    out["dist0"] = dist(start)
    for label, g in (("closed", gain), ("open", np.zeros_like(gain))):
        s = [v.copy() for v in start]
        ob = oracle.sim_ahead("cartpole", "euler", s, np.zeros((B, 0, 1)), props, E2E_TAU)[0][:, 0]
        biggest = 0.0
        for _ in range(E2E_STEPS):
            a = ff * (label == "closed") + np.einsum("bao,bo->ba", g, ob)
            biggest = max(biggest, float(np.abs(a).max()))
            ob, s = oracle.step("cartpole", "euler", s, np.clip(a, -1, 1), props, E2E_TAU)
        out["dist_" + label] = dist(s)
        if label == "closed":
            out["max_action"] = biggest
    return out
