"""Batched LQR synthesis on the GPU: excenv_lqr_backward (riccati_kernel) and `vmap_lqr` / `lqr_feedback` against the numpy twin of the
header's contract block (tests/helpers_lqr.py), bit for bit.

1. The grid: B in {1, 63, 64, 65, 326} x N in {0, 1, 2, 9} x the four (S, A) x fp32 / fp64 x q, r NULL / given x reg 0 / 0.25 x store_all
   0 / 1 x jac_row_stride 0 / dense, the C entry straight through ctypes. Every output (gain, ff, P0, p0, dV, n_bad) is bit-equal to the
   twin, a NaN standing for any NaN. One twin run of 9 rows on 326 lanes serves every B and N of a (shape, type, q / r, reg, stride):
   the lanes never mix, and the call over N rows is given the last N rows.
2. The same call twice, on copied inputs and on views offset by one element: the same bits.
3. An indefinite step (R = 0, a zero G row) is open loop and counted, a large enough reg mends it, a NaN in one environment's Jacobian
   stays in its lane: the twin's bits, and the counts.
4. `vmap_lqr` reads `vmap_linearize_ahead`'s buffer in place (pendulum, cart-pole; "step" semantics, B = 65, K = 9): bit-equal to the
   twin fed the downloaded Jacobians and to the same call on copied A, Bu.
5. End to end on cart-pole, fp64 and fp32, B = 64: `vmap_linearize` at the upright equilibrium, the stationary `vmap_lqr`,
   `lqr_feedback`, `vmap_sim_ahead_feedback`: every environment ends closer to the equilibrium than it started, no action reaches
   the clamp, and the zero-gain rollout from the same states ends further away. Perturbation, iterations and horizon are
   helpers_lqr.E2E_*, chosen on the CPU oracle (tests/test_lqr_host.py asserts the conditions there).
No division or sum turned out irreproducible: there is no exception to the bit equality."""
import numpy as np
import pytest
import torch

import helpers_lqr as hl
from helpers import make_env, to_state

pytestmark = pytest.mark.gpu
TORCH = {"float32": torch.float32, "float64": torch.float64}
REG = (0.0, 0.25)
OUTS = ("gain", "ff", "P0", "p0", "dV", "n_bad")


def _lane(x, dtype):
    """[B, ...] numpy -> [..., B] contiguous device tensor"""
    return torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(x), 0, -1)), dtype=dtype, device="cuda")


def _host(t):
    """[..., B] device tensor -> [B, ...] numpy"""
    return np.moveaxis(t.cpu().numpy(), -1, 0)


def _outputs(S, A, B, rows, dtype, fill=float("nan")):
    out = dict(gain=torch.full((rows, A, S, B), fill, dtype=dtype, device="cuda"), ff=torch.full((rows, A, B), fill, dtype=dtype, device="cuda"),
               P0=torch.full((S, S, B), fill, dtype=dtype, device="cuda"), p0=torch.full((S, B), fill, dtype=dtype, device="cuda"),
               dV=torch.full((2, B), fill, dtype=dtype, device="cuda"), n_bad=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
    return out


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run(S, A, B, N, dtype, jac, stride, Q, Qf, R, q, r, reg, store_all):
    """One excenv_lqr_backward call on device tensors (jac, q, r: from their first row on) -> the outputs as [B, ...] numpy"""
    rows = N if store_all else min(N, 1)
    out = _outputs(S, A, B, rows, dtype)
    spare = out["P0"]  # a call without rows writes no gain: the pointer only has to be there
    hl.raw_lqr(dtype, B, N, S, A, jac.data_ptr(), stride, Q.data_ptr(), _ptr(Qf), R.data_ptr(), _ptr(q), _ptr(r), reg, store_all,
               out["gain"].data_ptr() or spare.data_ptr(), out["ff"].data_ptr() or None, out["P0"].data_ptr(), out["p0"].data_ptr(),
               out["dV"].data_ptr(), out["n_bad"].data_ptr())
    torch.cuda.synchronize()
    got = {k: (_host(v) if k != "n_bad" else v.cpu().numpy()) for k, v in out.items()}
    return got


def _same(got, want, where):
    for k in OUTS:
        assert hl.same_bits(got[k], want[k]), (where, k, got[k].shape, want[k].shape)


def _grid(S, A, dtype):
    dt = TORCH[dtype]
    c = hl.grid_case(S, A, dtype)
    NM = hl.N_MAX
    Q, Qf, R = (torch.as_tensor(c[k], dtype=dt, device="cuda") for k in ("Q", "Qf", "R"))
    n = 0
    for B in hl.B_SIZES:
        jac = _lane(np.concatenate([c["F"][:B], c["G"][:B]], axis=-1), dt)  # [N, S, S + A, B]
        q, r = _lane(c["q"][:B], dt), _lane(c["r"][:B], dt)
        dense = S * (S + A) * B
        for with_lin in (False, True):
            for reg in REG:
                for invariant in (False, True):
                    twin = hl.grid_twin(S, A, dtype, with_lin, reg, invariant)
                    for N in hl.N_SIZES:
                        first = NM - N
                        j = jac[NM - 1] if invariant else jac[min(first, NM - 1):]
                        for store_all in (0, 1):
                            got = _run(S, A, B, N, dt, j, 0 if invariant else dense, Q, Qf, R, q[first:] if with_lin else None,
                                       r[min(first, NM - 1):] if with_lin else None, reg, store_all)
                            want = {k: v[:B] for k, v in twin.at(N, store_all).items()}
                            _same(got, want, (B, N, with_lin, reg, invariant, store_all))
                            n += 1
    # Qf == NULL means Q
    B, N = 65, 2
    jac = _lane(np.concatenate([c["F"][:B, -N:], c["G"][:B, -N:]], axis=-1), dt)
    got = _run(S, A, B, N, dt, jac, S * (S + A) * B, Q, None, R, None, None, 0.0, 1)
    tw = hl.lqr_twin(c["F"][:B, -N:], c["G"][:B, -N:], c["Q"], c["R"], dtype=dtype)
    _same(got, tw.at(N), "Qf NULL")
    print(f"riccati_kernel S={S} A={A} {dtype}: {n + 1} calls, every output bit-equal to the twin")


def _runs_and_layouts(S, A, dtype):
    dt = TORCH[dtype]
    c = hl.grid_case(S, A, dtype)
    B, N = 65, hl.N_MAX
    Q, Qf, R = (torch.as_tensor(c[k], dtype=dt, device="cuda") for k in ("Q", "Qf", "R"))
    jac = _lane(np.concatenate([c["F"][:B], c["G"][:B]], axis=-1), dt)
    q, r = _lane(c["q"][:B], dt), _lane(c["r"][:B], dt)
    dense = S * (S + A) * B
    ref = _run(S, A, B, N, dt, jac, dense, Q, Qf, R, q, r, 0.25, 1)
    _same(_run(S, A, B, N, dt, jac, dense, Q, Qf, R, q, r, 0.25, 1), ref, "second run")
    _same(_run(S, A, B, N, dt, jac.clone(), dense, Q.clone(), Qf.clone(), R.clone(), q.clone(), r.clone(), 0.25, 1), ref, "copied inputs")

    def shifted(t):  # the same values one element off the allocation's start
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(t.shape)

    _same(_run(S, A, B, N, dt, shifted(jac), dense, shifted(Q), shifted(Qf), shifted(R), shifted(q), shifted(r), 0.25, 1), ref, "offset views")
    # a padded row stride: the rows one element further apart
    padded = torch.zeros((N, dense + 1), dtype=dt, device="cuda")
    padded[:, :dense].copy_(jac.reshape(N, dense))
    _same(_run(S, A, B, N, dt, padded, dense + 1, Q, Qf, R, q, r, 0.25, 1), ref, "padded stride")


def _indefinite_and_nan(dtype):
    dt = TORCH[dtype]
    S, A, B, N = 4, 1, 5, 4
    c = hl.rounded(hl.random_problem(S, A, B, N, seed=9), dtype)
    G0 = c["G"].copy()
    G0[:, 2] = 0.0
    R0 = np.zeros((A, A))
    Fn = c["F"].copy()
    Fn[3, 1, 0, 0] = np.nan
    dev = lambda x: torch.as_tensor(x, dtype=dt, device="cuda")

    def run(F, G, R, reg):
        jac = _lane(np.concatenate([F, G], axis=-1), dt)
        got = _run(S, A, B, N, dt, jac, S * (S + A) * B, dev(c["Q"]), dev(c["Qf"]), dev(R), _lane(c["q"], dt), _lane(c["r"], dt), reg, 1)
        tw = hl.lqr_twin(F, G, c["Q"], R, Qf=c["Qf"], q=c["q"], r=c["r"], reg=reg, dtype=dtype)
        _same(got, tw.at(N), (reg,))
        return got

    bad = run(c["F"], G0, R0, 0.0)
    assert (bad["n_bad"] == 1).all() and not bad["gain"][:, 2].any() and not bad["ff"][:, 2].any() and bad["gain"][:, 1].any()
    mended = run(c["F"], G0, R0, 0.5)
    assert not mended["n_bad"].any() and mended["ff"][:, 2].all()
    ref = run(c["F"], c["G"], c["R"], 0.0)
    nan = run(Fn, c["G"], c["R"], 0.0)
    others = [b for b in range(B) if b != 3]
    assert nan["n_bad"][3] == 1 and not nan["n_bad"][others].any() and np.isnan(nan["P0"][3]).all()
    for k in OUTS:
        assert hl.same_bits(nan[k][others], ref[k][others]), k


def _in_place(env_name, dtype):
    dt = TORCH[dtype]
    B, K = 65, 9
    env, _, _, spec = make_env(env_name, B, dt)
    env.sim_ahead_semantics = "step"
    S, A = env.physical_state_dim, env.action_dim
    rng = np.random.default_rng(21)
    from helpers import random_state

    state = to_state(env, random_state(env_name, B, np.float64, spec, 21))
    actions = torch.as_tensor(rng.uniform(-1, 1, (B, K, A)), dtype=dt, device="cuda")
    _, states, _ = env.vmap_sim_ahead(state, actions, env.tau, env.tau)
    Aj, Bj = env.vmap_linearize_ahead(states, actions, env.tau, env.tau)
    Q, R = np.diag(np.arange(1.0, S + 1.0)), np.array([[0.5]])
    q, r = rng.uniform(-1, 1, (B, K + 1, S)), rng.uniform(-1, 1, (B, K, A))
    sol = env.vmap_lqr(Aj, Bj, Q, R, q=q, r=r, reg=0.125)
    assert env.last_lqr_launch == "riccati_kernel" and env.last_lqr_in_place
    assert tuple(sol.gain.shape) == (B, K, A, S) and tuple(sol.feedforward.shape) == (B, K, A) and tuple(sol.value_hessian.shape) == (B, S, S)
    assert tuple(sol.value_gradient.shape) == (B, S) and tuple(sol.expected_change.shape) == (B, 2) and tuple(sol.n_bad.shape) == (B,)
    assert not any(t.requires_grad for t in sol)
    tw = hl.lqr_twin(Aj.cpu().numpy(), Bj.cpu().numpy(), Q, R, q=q, r=r, reg=0.125, dtype=dtype).at(K)
    got = dict(zip(OUTS, (t.cpu().numpy() for t in sol)))
    _same(got, tw, "in place")
    again = env.vmap_lqr(Aj.clone(), Bj.clone(), Q, R, q=torch.as_tensor(q), r=torch.as_tensor(r), reg=0.125)
    assert not env.last_lqr_in_place
    _same(dict(zip(OUTS, (t.cpu().numpy() for t in again))), got, "copied A, Bu")
    # the stationary use on one row of the same buffer, and a horizon of no rows
    one = env.vmap_lqr(Aj[:, 0], Bj[:, 0], Q, R, n_iter=5)
    assert env.last_lqr_in_place and tuple(one.gain.shape) == (B, 1, A, S)
    tw1 = hl.lqr_twin(Aj[:, 0].cpu().numpy(), Bj[:, 0].cpu().numpy(), Q, R, dtype=dtype, n_iter=5).at(5, store_all=0)
    _same(dict(zip(OUTS, (t.cpu().numpy() for t in one))), tw1, "stationary")
    none = env.vmap_lqr(Aj[:, :0], Bj[:, :0], Q, R, Qf=2 * Q, q=q[:, :1])
    assert tuple(none.gain.shape) == (B, 0, A, S) and not none.n_bad.any() and not none.expected_change.any()
    assert torch.equal(none.value_hessian, torch.as_tensor(2 * Q, dtype=dt, device="cuda").expand(B, S, S))
    assert torch.equal(none.value_gradient, torch.as_tensor(q[:, 0], dtype=dt, device="cuda"))


def _regulated(dtype):
    dt = TORCH[dtype]
    B, K = hl.E2E_B, hl.E2E_STEPS
    env, _, _, spec = make_env("cartpole", B, dt, spec=hl.cartpole_spec())
    env.sim_ahead_semantics = "step"
    S, A = env.physical_state_dim, env.action_dim
    upright = to_state(env, [np.zeros(B)] * S)
    Aj, Bj = env.vmap_linearize(upright, torch.zeros((B, A), dtype=dt, device="cuda"))
    sol = env.vmap_lqr(Aj, Bj, hl.E2E_Q, hl.E2E_R, n_iter=hl.E2E_ITERS)
    assert env.last_lqr_in_place and not sol.n_bad.any()
    ref = hl.cartpole_reference()
    Kg = sol.gain[:, 0]
    print("stationary gain:", Kg[0].cpu().numpy(), "CPU reference:", ref["K"])
    gain, ff = env.lqr_feedback(Kg, torch.zeros(S), torch.zeros(A))
    start = hl.cartpole_start()
    state = to_state(env, start)
    dist0 = np.sqrt(sum(v * v for v in start))
    tau = spec["tau"]
    _, _, last, acts, _ = env.vmap_sim_ahead_feedback(state, gain, K, tau, tau, feedforward=ff[:, None, :].expand(B, K, A))
    _, _, last0, acts0, _ = env.vmap_sim_ahead_feedback(state, torch.zeros_like(gain), K, tau, tau)
    dist = lambda st: np.sqrt(sum(getattr(st.physical_state, n).double().cpu().numpy() ** 2 for n in env.STATE_FIELDS))
    closed, opened = dist(last), dist(last0)
    biggest = float(acts.abs().max())
    print(f"{dtype}: largest |action| {biggest:.3f}; final / initial distance at most {float((closed / dist0).max()):.3g} closed loop, "
          f"at least {float((opened / dist0).min()):.3g} with zero gain")
    assert biggest < 1.0  # the clamp at +-1 was never reached
    assert (closed < dist0).all()
    assert (opened > dist0).all() and not acts0.any()


# ---- the tests: one per property, each looping over its shapes and types (a second or two in all) ---------------------------------------
def test_every_output_equals_the_twin_bit_for_bit_on_every_run_and_layout():
    for S, A in hl.SHAPES:
        for dtype in hl.DTYPES:
            _grid(S, A, dtype)
            if (S, A) in ((4, 1), (7, 2)):
                _runs_and_layouts(S, A, dtype)


def test_indefinite_step_and_nan_lane():
    for dtype in hl.DTYPES:
        _indefinite_and_nan(dtype)


def test_vmap_lqr_reads_the_linearisation_in_place():
    for env_name in ("pendulum", "cartpole"):
        for dtype in hl.DTYPES:
            _in_place(env_name, dtype)


def test_cartpole_is_regulated_end_to_end():
    for dtype in hl.DTYPES:
        _regulated(dtype)
