"""Host side of the batched LQR synthesis (excenv_lqr_backward; `vmap_lqr`, `lqr_feedback`; no GPU):
- the header with the contract block and its `_native` mirror, the exports, ABI 7; the eight instantiations without scratch memory;
- every refusal by code and whole message, before any launch; B == 0 returns OK; the bytes function against a restatement;
- the twin (helpers_lqr.lqr_twin) against an independent solution: the open-loop optimum of the stacked problem from
  numpy.linalg.solve equals the closed loop under the twin's gains, and the value function at row 0 gives the optimal cost;
- the stationary mode: the residual of the discrete algebraic Riccati equation falls with every doubling of the iterations;
- an indefinite step is open loop and counted, a large enough `reg` mends it, a NaN stays in its own lane;
- `lqr_feedback` against u_ref + K (x - x_ref) on random states inside the bounds; what the Python methods refuse."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_lqr as hl
from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64 = ctypes.c_int64
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
FN = "excenv_lqr_backward"
EPS64 = 2.0 ** -52
# Twin against the stacked solution, measured over the cases of test_twin_equals_the_stacked_optimum (float64): the largest ratio
# error / (eps64 cond(H) |U|) was 19.9 for the inputs ((S, A) = (4, 1); 3.0, 3.2 and 2.3 for the other shapes) and 96.6 for the cost
# ((2, 1); 9.6, 26.4, 8.8), whose error is measured in the bound of the inputs although it scales with the cost. One c for both: the
# larger ratio times a margin of 10, rounded up.
C_STACKED = 1000.0


def test_header_declares_the_contract_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)
    for fn in (FN, FN + "_bytes"):
        assert re.search(rf"\b{fn}\s*\(", hdr), fn
    assert re.search(r"\}\s*excenv_lqr_t\s*;", hdr)
    for line in ("W[i][j]   = P[i][0] * F[0][j];   k >= 1: W[i][j]  = fma(P[i][k], F[k][j], W[i][j])",
                 "Qxx[i][j] = Q[i][j];             k: Qxx[i][j] = fma(F[k][i], W[k][j], Qxx[i][j])",
                 "Quu[a][c] = R[a][c];             k: Quu[a][c] = fma(G[k][a], Wb[k][c], Quu[a][c])",
                 "A = 2:  d0 = Quu[0][0] + reg;  l = Quu[0][1] / d0;  d1 = fma(-l, Quu[0][1], Quu[1][1] + reg);  ok = d0 > 0 && d1 > 0",
                 "y1 = fma(-l, g0, g1);  x1 = y1 / d1;  x0 = fma(-l, x1, g0 / d0)",
                 "if !ok:  K = 0, k = 0, bad += 1",
                 "a: dV0 = fma(k[a], Qu[a], dV0);   h = k[0] * Qk[0];  A = 2: h = fma(k[1], Qk[1], h);   dV1 = dV1 + 0.5 * h"):
        assert line in hdr, line
    lib = ctypes.CDLL(_native.library_path())
    for fn in (FN, FN + "_bytes"):
        assert hasattr(lib, fn) and fn in _native.PROTOTYPES, fn
    assert _native.lib().excenv_abi_version() == 7
    assert _native.STRUCTS[_native.Lqr] == "excenv_lqr_t"
    assert [n for n, _ in _native.Lqr._fields_] == ["n_state", "n_action", "jac", "jac_row_stride", "Q", "Qf", "R", "q", "r", "reg", "store_all",
                                                    "gain", "ff", "P0", "p0", "dV", "n_bad"]
    assert _native.LQR_SHAPES == hl.SHAPES
    assert excenvs.LQRSolution._fields == ("gain", "feedforward", "value_hessian", "value_gradient", "expected_change", "n_bad")
    assert "LQRSolution" in excenvs.__all__
    for method in ("vmap_lqr", "lqr_feedback"):
        assert callable(getattr(excenvs.CoreEnvironment, method))


def test_eight_instantiations_without_scratch():
    res, _ = budget("riccati_kernel")
    for t in "fd":
        for S, A in hl.SHAPES:
            hit = [k for k in res if f"riccati_kernelI{t}Li{S}ELi{A}E" in k]
            assert len(hit) == 1, (t, S, A, hit)
            print(hit[0], res[hit[0]])
    assert len(res) == 8, sorted(res)
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in res.values()), res


def _record(**kw):
    r = _native.Lqr(2, 1, 64, 0, 64, 64, 64, 64, 64, 0.0, 1, 64, 64, 64, 64, 64, 64)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(rec, dtype=0, B=4, N=3, no_rec=False):
    lib = _native.lib()
    rc = lib.excenv_lqr_backward(dtype, i64(B), i64(N), None if no_rec else ctypes.byref(rec), None)
    return rc, lib.excenv_last_error().decode()


def test_refusals_by_code_and_whole_message():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    assert _call(None, no_rec=True) == (ENULL, f"{FN}: call is NULL")
    for field in ("jac", "Q", "R", "gain"):
        assert _call(_record(**{field: None})) == (ENULL, f"{FN}: call->{field} is NULL")
    assert _call(_record(), dtype=2) == (EINVAL, f"{FN}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(_record(), B=-1) == (EINVAL, f"{FN}: bad B=-1 or N=3")
    assert _call(_record(), N=-2) == (EINVAL, f"{FN}: bad B=4 or N=-2")
    for S, A in ((3, 1), (2, 2), (7, 1), (0, 1), (4, 0), (8, 2), (-1, 1)):
        assert _call(_record(n_state=S, n_action=A)) == (
            EUNSUPPORTED, f"{FN}: no riccati_kernel for n_state={S}, n_action={A}: the shapes are (1, 1), (2, 1), (4, 1) and (7, 2)")
    assert _call(_record(reg=-1e-300)) == (EINVAL, f"{FN}: call->reg must not be negative or NaN (got -1e-300)")
    assert _call(_record(reg=float("nan")))[0] == EINVAL and "must not be negative or NaN" in _call(_record(reg=float("nan")))[1]
    for v in (2, -1):
        assert _call(_record(store_all=v)) == (EINVAL, f"{FN}: call->store_all must be 0 or 1 (got {v})")
    for S, A, B in ((2, 1, 4), (7, 2, 326), (1, 1, 1)):
        need = S * (S + A) * B
        for stride in (need - 1, 1, -need):
            assert _call(_record(n_state=S, n_action=A, jac_row_stride=stride), B=B) == (
                EINVAL, f"{FN}: call->jac_row_stride must be 0 or at least S (S + A) B = {need} (got {stride})")
    assert _call(_record(), B=1 << 39) == (EUNSUPPORTED, f"{FN}: batch too large for one launch")
    assert _call(_record(jac=None, n_state=99), dtype=2) == (ENULL, f"{FN}: call->jac is NULL")  # NULL pointers come first
    # B == 0: EXCENV_OK without a launch, whatever N and the optional pointers
    for rec in (_record(), _record(Qf=None, q=None, r=None, ff=None, P0=None, p0=None, dV=None, n_bad=None), _record(n_state=7, n_action=2, store_all=0)):
        assert _call(rec, B=0)[0] == 0 and _call(rec, B=0, N=0, dtype=1)[0] == 0
    assert _call(_record(gain=None), B=0)[0] == ENULL


def test_bytes_function_equals_its_restatement():
    lib = _native.lib()
    n = 0
    for d, dtype in enumerate(hl.DTYPES):
        for S, A in hl.SHAPES:
            for flags in range(32):
                ti, hq, hr, sa, hf = [(flags >> k) & 1 for k in range(5)]
                assert lib.excenv_lqr_backward_bytes(d, S, A, ti, hq, hr, sa, hf) == hl.bytes_per_row(dtype, S, A, ti, hq, hr, sa, hf)
                n += 1
    assert lib.excenv_lqr_backward_bytes(0, 7, 2, 0, 1, 1, 1, 1) == 4 * (63 + 7 + 2 + 14 + 2) and n == 256
    assert lib.excenv_lqr_backward_bytes(2, 2, 1, 0, 0, 0, 1, 1) == -1 and lib.excenv_lqr_backward_bytes(0, 3, 1, 0, 0, 0, 1, 1) == -1


# ---- the twin against an independent solution ------------------------------------------------------------------------------------
def _stacked(F, G, Q, Qf, R, q, r, x0):
    """One environment's problem with the states eliminated: x = Sx x0 + Su U stacks x_1 .. x_N, the cost becomes
    U^T H U / 2 + g . U + const with H = Su^T Qbar Su + Rbar. -> (H, g, cost(U))"""
    N, S, A = F.shape[0], F.shape[-1], G.shape[-1]
    Sx, Su = np.zeros((N * S, S)), np.zeros((N * S, N * A))
    Phi = np.eye(S)
    for n in range(N):
        Phi = F[n] @ Phi
        Sx[n * S:(n + 1) * S] = Phi
        for m in range(n + 1):
            blk = G[m]
            for k in range(m + 1, n + 1):
                blk = F[k] @ blk
            Su[n * S:(n + 1) * S, m * A:(m + 1) * A] = blk
    Qbar = np.zeros((N * S, N * S))
    for n in range(N):
        Qbar[n * S:(n + 1) * S, n * S:(n + 1) * S] = Q if n < N - 1 else Qf
    Rbar = np.kron(np.eye(N), R)
    qbar, rbar = q[1:].reshape(-1), r.reshape(-1)
    H = Su.T @ Qbar @ Su + Rbar
    g = Su.T @ (Qbar @ (Sx @ x0) + qbar) + rbar

    def cost(U):
        x = np.concatenate([x0, Sx @ x0 + Su @ U]).reshape(N + 1, S)
        u = U.reshape(N, A)
        J = 0.5 * x[N] @ Qf @ x[N] + q[N] @ x[N]
        for n in range(N):
            J += 0.5 * x[n] @ Q @ x[n] + q[n] @ x[n] + 0.5 * u[n] @ R @ u[n] + r[n] @ u[n]
        return J

    return H, g, cost


@pytest.mark.parametrize("S,A", hl.SHAPES)
def test_twin_equals_the_stacked_optimum(S, A):
    """float64. The stationarity condition of the stacked problem, H U = -g, solved with numpy.linalg.solve, against the closed loop
    u_n = k_n + K_n x_n under the twin's gains from the same x_0; and x_0^T P0 x_0 / 2 + p0 . x_0 + dV0 + dV1 against the optimal cost.
    Both within C_STACKED eps64 cond(H) |U|."""
    B = 6
    worst_u = worst_j = 0.0
    for N in (1, 2, 9):
        for with_lin in (False, True):
            c = hl.random_problem(S, A, B, N, seed=N + 10 * with_lin)
            q, r = (c["q"], c["r"]) if with_lin else (np.zeros_like(c["q"]), np.zeros_like(c["r"]))
            tw = hl.lqr_twin(c["F"], c["G"], c["Q"], c["R"], Qf=c["Qf"], q=q if with_lin else None, r=r if with_lin else None)
            sol = tw.at(N)
            assert not sol["n_bad"].any()
            x0s = np.random.default_rng(77 + N).normal(0.0, 1.0, (B, S))
            for b in range(B):
                H, g, cost = _stacked(c["F"][b], c["G"][b], c["Q"], c["Qf"], c["R"], q[b], r[b], x0s[b])
                U = np.linalg.solve(H, -g)
                x, u = x0s[b].copy(), []
                for n in range(N):
                    u.append(sol["ff"][b, n] + sol["gain"][b, n] @ x)
                    x = c["F"][b, n] @ x + c["G"][b, n] @ u[-1]
                u = np.concatenate(u)
                bound = EPS64 * np.linalg.cond(H) * np.linalg.norm(U)
                err_u = np.linalg.norm(u - U)
                J = 0.5 * x0s[b] @ sol["P0"][b] @ x0s[b] + sol["p0"][b] @ x0s[b] + sol["dV"][b, 0] + sol["dV"][b, 1]
                err_j = abs(J - cost(U))
                worst_u, worst_j = max(worst_u, err_u / bound), max(worst_j, err_j / bound)
                assert err_u <= C_STACKED * bound, (N, with_lin, b, err_u, bound)
                assert err_j <= C_STACKED * bound, (N, with_lin, b, err_j, bound)
    print(f"twin vs stacked optimum S={S} A={A}: error / (eps64 cond(H) |U|) at most {worst_u:.3g} (inputs), {worst_j:.3g} (cost)")


@pytest.mark.parametrize("S,A", hl.SHAPES)
def test_stationary_mode_converges_to_the_algebraic_riccati_equation(S, A):
    """jac_row_stride = 0 on a controllable pair: the residual of P = Q + F^T P F - F^T P G (R + G^T P G)^-1 G^T P F at the twin's P0 falls
    from N to 2 N, for every doubling from 1 to 8 (at 16 the fastest draw is at the rounding floor of float64)."""
    c = hl.random_problem(S, A, 3, 1, seed=5)
    F, G = c["F"][:, 0], c["G"][:, 0]
    tw = hl.lqr_twin(F, G, c["Q"], c["R"], n_iter=8)
    res = []
    for N in (1, 2, 4, 8):
        P = tw.P[N]
        FtPG = np.einsum("bki,bkl,bla->bia", F, P, G)
        rhs = c["Q"] + np.einsum("bki,bkl,blj->bij", F, P, F) - FtPG @ np.linalg.solve(c["R"] + np.einsum("bka,bkl,blc->bac", G, P, G), FtPG.transpose(0, 2, 1))
        res.append(np.abs(P - rhs).max(axis=(1, 2)))
    res = np.array(res)
    print("DARE residual by N:", res.max(axis=1))
    assert (res[1:] < res[:-1]).all(), res


def test_indefinite_step_is_open_loop_and_counted_and_reg_mends_it():
    S, A, B, N = 4, 1, 5, 4
    c = hl.random_problem(S, A, B, N, seed=9)
    G = c["G"].copy()
    G[:, 2] = 0.0  # with R = 0: Quu = 0 at row 2
    R0 = np.zeros((A, A))
    for dtype in hl.DTYPES:
        tw = hl.lqr_twin(c["F"], G, c["Q"], R0, Qf=c["Qf"], q=c["q"], r=c["r"], dtype=dtype)
        assert (tw.n_bad[N] == 1).all() and (tw.n_bad[1] == 0).all() and (tw.n_bad[2] == 1).all()
        assert (tw.gain[:, 2] == 0).all() and (tw.ff[:, 2] == 0).all() and (tw.gain[:, 1] != 0).any()
        # P continues as Qxx = Q + F^T P F of that row
        t = np.dtype(dtype).type
        Fr, Pn = c["F"][:, 2].astype(t).astype(np.float64), tw.P[1].astype(np.float64)
        Qxx = c["Q"] + np.einsum("bki,bkl,blj->bij", Fr, Pn, Fr)
        assert np.allclose(tw.P[2], Qxx, rtol=64 * np.finfo(t).eps, atol=0)
        mended = hl.lqr_twin(c["F"], G, c["Q"], R0, Qf=c["Qf"], q=c["q"], r=c["r"], reg=0.5, dtype=dtype)
        assert (mended.n_bad[N] == 0).all() and (mended.ff[:, 2] != 0).all()
        # a NaN in one environment's Jacobian: its own n_bad and outputs, no other lane
        Fn = c["F"].copy()
        Fn[3, 1, 0, 0] = np.nan
        ref = hl.lqr_twin(c["F"], c["G"], c["Q"], c["R"], Qf=c["Qf"], q=c["q"], r=c["r"], dtype=dtype)
        nan = hl.lqr_twin(Fn, c["G"], c["Q"], c["R"], Qf=c["Qf"], q=c["q"], r=c["r"], dtype=dtype)
        others = [b for b in range(B) if b != 3]
        assert nan.n_bad[N][3] == 1 and not nan.n_bad[N][others].any() and np.isnan(nan.P[N][3]).all()
        for name in ("gain", "ff"):
            assert hl.same_bits(getattr(nan, name)[others], getattr(ref, name)[others])
        assert hl.same_bits(nan.P[N][others], ref.P[N][others]) and hl.same_bits(nan.dV[N][others], ref.dV[N][others])
        assert hl.same_bits(nan.gain[3, 2:], ref.gain[3, 2:])  # the rows behind the NaN are untouched


# ---- the Python methods -------------------------------------------------------------------------------------------------------------
AFFINE = ("PENDULUM", "MASS_SPRING_DAMPER", "CART_POLE", "ACROBOT", "FLUID_TANK")


def _env(name, B, dtype=torch.float64, **kw):
    return getattr(EnvironmentRegistry, name).make(batch_size=B, dtype=dtype, device="cpu", **kw)


@pytest.mark.parametrize("name", AFFINE)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_lqr_feedback_equals_the_state_feedback(name, dtype):
    """feedforward + gain @ obs_row against u_ref + K (x - x_ref) in float64 numpy on random states inside the bounds. Each side is a
    short sum of S + 1 (+ the bias terms) products: the bound is 4 eps sum |terms| in the working dtype, the terms being those of
    both sides."""
    B = 7
    env = _env(name, B, dtype)
    ctrl = _env(name, B, dtype, control_state=[env.STATE_FIELDS[0]])
    rng = np.random.default_rng(11)
    for e in (env, ctrl):
        S, A, OW = e.physical_state_dim, e.action_dim, e._obs_dim()
        pn = e.env_properties.physical_normalizations
        lo = np.array([float(getattr(pn, n).min) for n in e.STATE_FIELDS])
        hi = np.array([float(getattr(pn, n).max) for n in e.STATE_FIELDS])
        K = rng.normal(0.0, 1.0, (B, A, S)) / (hi - lo)
        x_ref = lo + rng.uniform(0.3, 0.7, (B, S)) * (hi - lo)
        u_ref = rng.uniform(-0.3, 0.3, (B, A))
        x = lo + rng.uniform(0.0, 1.0, (B, S)) * (hi - lo)
        npdt = np.float32 if dtype == torch.float32 else np.float64
        K, x_ref, u_ref, x = (v.astype(npdt).astype(np.float64) for v in (K, x_ref, u_ref, x))
        gain, ff = e.lqr_feedback(torch.as_tensor(K), torch.as_tensor(x_ref), torch.as_tensor(u_ref))
        assert tuple(gain.shape) == (B, A, OW) and tuple(ff.shape) == (B, A) and gain.dtype == dtype
        assert not gain[:, :, S:].any()  # the columns of controlled references
        obs = np.zeros((B, OW))
        obs[:, :S] = 2 * (x - lo) / (hi - lo) - 1
        obs[:, S:] = rng.uniform(-1, 1, (B, OW - S))
        got = ff.double().numpy() + np.einsum("bao,bo->ba", gain.double().numpy(), obs)
        want = u_ref + np.einsum("bas,bs->ba", K, x - x_ref)
        half = (hi - lo) / 2
        terms = (np.abs(u_ref) + np.einsum("bas,bs->ba", np.abs(K), np.abs(x) + np.abs(x_ref))
                 + np.einsum("bas,bs->ba", np.abs(K), half * np.abs(obs[:, :S]) + np.abs(lo + half) + np.abs(x_ref)))
        err = np.abs(got - want)
        print(name, dtype, "largest error / (eps sum|terms|):", float((err / (np.finfo(npdt).eps * terms)).max()))
        assert (err <= 4 * np.finfo(npdt).eps * terms).all()
        # one gain set for all environments broadcasts
        g1, f1 = e.lqr_feedback(torch.as_tensor(K[0]), torch.as_tensor(x_ref[0]), torch.as_tensor(u_ref[0]))
        assert torch.equal(g1[0], gain[0]) and torch.equal(f1[0], ff[0]) and tuple(g1.shape) == (B, A, OW)


def test_python_methods_refuse_by_name():
    env = _env("CART_POLE", 3)
    pmsm = _env("PMSM", 3)
    with pytest.raises(ValueError, match="lqr_feedback: the PMSM's observation"):
        pmsm.lqr_feedback(torch.zeros(2, 7), torch.zeros(7), torch.zeros(2))
    with pytest.raises(ValueError, match=r"lqr_feedback: K needs to be of shape \(1, 4\) or \(3, 1, 4\)"):
        env.lqr_feedback(torch.zeros(4), torch.zeros(4), torch.zeros(1))
    with pytest.raises(ValueError, match=r"lqr_feedback: x_ref needs to be of shape"):
        env.lqr_feedback(torch.zeros(1, 4), torch.zeros(3), torch.zeros(1))
    F, G, Q, R = torch.zeros(3, 5, 4, 4), torch.zeros(3, 5, 4, 1), torch.eye(4), torch.eye(1)
    with pytest.raises(ValueError, match="vmap_lqr: reg needs to be a non-negative number"):
        env.vmap_lqr(F, G, Q, R, reg=-1.0)
    with pytest.raises(ValueError, match="vmap_lqr: reg needs to be a non-negative number"):
        env.vmap_lqr(F, G, Q, R, reg=float("nan"))
    with pytest.raises(ValueError, match="vmap_lqr: A and Bu need to be of shape"):
        env.vmap_lqr(F, G[:, :4], Q, R)
    with pytest.raises(ValueError, match="vmap_lqr: n_iter goes with"):
        env.vmap_lqr(F, G, Q, R, n_iter=3)
    with pytest.raises(ValueError, match="stationary use, which needs n_iter"):
        env.vmap_lqr(F[:, 0], G[:, 0], Q, R)
    with pytest.raises(ValueError, match="vmap_lqr: Q needs to be symmetric"):
        env.vmap_lqr(F, G, torch.triu(torch.ones(4, 4)), R)
    with pytest.raises(ValueError, match=r"vmap_lqr: R needs to be of shape \(1, 1\)"):
        env.vmap_lqr(F, G, Q, torch.eye(2))
    with pytest.raises(ValueError, match=r"vmap_lqr: q needs to be of shape \(3, 6, 4\)"):
        env.vmap_lqr(F, G, Q, R, q=torch.zeros(3, 5, 4))
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
        env.vmap_lqr(F, G, Q, R)  # a CPU environment reaches the launch and is refused there: there is no CPU path


def test_cartpole_reference_satisfies_the_end_to_end_conditions():
    """The chain of tests/test_gpu_lqr.py's end-to-end case on the CPU oracle in float64, with the recorded perturbation size, Riccati
    iterations and horizon (helpers_lqr.E2E_*): every environment ends closer to the equilibrium than it started, the same states
    under zero gain end further away, and no action reaches the clamp."""
    ref = hl.cartpole_reference()
    print("K =", ref["K"], "largest |action|:", ref["max_action"], "closed final / initial at most", float((ref["dist_closed"] / ref["dist0"]).max()),
          "open final / initial at least", float((ref["dist_open"] / ref["dist0"]).min()))
    assert ref["max_action"] < 1.0
    assert (ref["dist_closed"] < ref["dist0"]).all() and (ref["dist_open"] > ref["dist0"]).all()
    assert (ref["dist0"] > 0).all()
