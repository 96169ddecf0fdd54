"""Batched linearisation on the GPU: `vmap_linearize` / `vmap_linearize_ahead` (step_jac_kernel through excenv_step_jacobian)
against the float64 torch twin of tests/helpers_vjp.py, against the existing reverse-mode step and trajectory kernels, and at the edges.

Every case runs at B = 257 (one workgroup plus a one-lane tail) unless it says otherwise. Bounds: helpers_vjp.rel_dist, relative to each
compared tensor's largest magnitude (A = d row / d state and Bu = d row / d action are the two tensors of a Jacobian).
1. fp64 kernel vs the twin's Jacobian (one-hot cotangents through twin_step / twin_step_grads): 1e-8, both row kinds, one PMSM case
   with controlled currents (the observation then has reference columns, and R = O leaves them out).
2. fp32 kernel vs the twin: 32 x the forward floor (obs_floor of the fp32 forward vmap_step, code this kernel does not touch);
   environments the twin sees within KINK_MARGIN of a kink are excluded, at most KINK_CAP of them (tests/test_linearize_host.py
   asserts the cap on the same inputs without a GPU).
3. vmap_linearize vs S calls of vmap_step_vjp with one-hot grad_state: 2e-8 in fp64 (each side holds 1e-8 to the twin); bit equality
   is printed, not asserted.
4. vmap_linearize_ahead, substeps = 1, K = 4: row n is torch.equal to vmap_linearize on that row — the same kernel on the same
   operands, any difference is an indexing bug. Lane-major actions and a plain contiguous [B, K, A] tensor.
5. vmap_linearize_ahead, substeps = 2 (K = 3, N = 6), against the trajectory reverse kernel: the cotangent carried back through the
   Jacobians equals vmap_sim_ahead_vjp(grad_last_state=g_last) within 2e-8.
6. Edges: B = 1, B = 63, empty batches and trajectories, an action slice off a 16-byte boundary, no grad_fn, the launch's name.
Every case prints its figures."""
import numpy as np
import pytest
import torch

from helpers import make_env, to_state
from helpers_step_vjp import B0, SEED, step_inputs, twin_step, twin_step_grads
from helpers_vjp import CASES, KINK_CAP, KINK_MARGIN, SOLVERS, GpuRun, dev, obs_floor, rel_dist, skewed_spec, vjp_inputs

pytestmark = pytest.mark.gpu

NAMES = {"state": "step_jac_kernel (V=1, state rows)", "obs": "step_jac_kernel (V=1, observation rows)"}
F64 = torch.float64


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _leaves(env, state):
    return [getattr(state.physical_state, n) for n in env.STATE_FIELDS]


_TWIN = {}


def _twin_jacobians(env_name, deadtime, solver, npd, B=B0):
    """The twin's Jacobians of one step on step_inputs (computed once per case and shared, never modified) ->
    {"state": (A [B, S, S], Bu [B, S, A]), "obs": (A [B, O, S], Bu [B, O, A])}, forward observation [B, O], kept environments [B]"""
    key = (env_name, deadtime, solver, npd, B)
    if key not in _TWIN:
        spec, st, act = step_inputs(env_name, deadtime, B, SEED, npd)
        st64, act64 = [np.asarray(v, dtype=np.float64) for v in st], np.asarray(act, dtype=np.float64)
        tw = twin_step(env_name, spec, solver, st64, act64)
        S, O = len(st64), tw[2].shape[1]
        out = {}
        for kind, R in (("state", S), ("obs", O)):
            a_rows, b_rows = [], []
            for r in range(R):
                if kind == "state":
                    ga, gs = twin_step_grads(tw, g_state=[np.ones(B) if j == r else None for j in range(S)])
                else:
                    e = np.zeros((B, O))
                    e[:, r] = 1.0
                    ga, gs = twin_step_grads(tw, g_obs=e)
                a_rows.append(np.stack(gs, axis=-1))
                b_rows.append(ga)
            out[kind] = (np.stack(a_rows, axis=1), np.stack(b_rows, axis=1))
        kd = tw[5]
        keep = np.ones(B, dtype=bool) if kd is None else (kd.numpy() >= KINK_MARGIN)
        _TWIN[key] = (out, tw[2].detach().numpy(), keep, spec, st, act)
    return _TWIN[key]


def _setup(env_name, deadtime, solver, dtype, B=B0, control=()):
    npd = np.float32 if dtype is torch.float32 else np.float64
    want, obs64, keep, spec, st, act = _twin_jacobians(env_name, deadtime, solver, npd, B)
    env, _, _, _ = make_env(env_name, B, dtype, solver, spec=spec, control_state=list(control))
    return env, to_state(env, st), dev(act, env), want, obs64, keep


def _check_shapes(env, A, Bu, R, lead):
    S, NA = env.physical_state_dim, env.action_dim
    assert tuple(A.shape) == lead + (R, S) and tuple(Bu.shape) == lead + (R, NA)
    assert A.grad_fn is None and Bu.grad_fn is None and not A.requires_grad and not Bu.requires_grad
    assert A.dtype is env.dtype and A.device == Bu.device
    if A.numel() and Bu.numel():  # views of one lane-major allocation
        assert A.stride(0) == 1 and Bu.stride(0) == 1 and A.untyped_storage().data_ptr() == Bu.untyped_storage().data_ptr()


# ---------------------------------------------------------------------------------------------------------------- 1
def _fp64_vs_twin(env_name, deadtime, solver, B=B0, control=()):
    env, state, action, want, _, _ = _setup(env_name, deadtime, solver, F64, B, control)
    _, new_state = env.vmap_step(state, action)
    for kind in ("state", "obs"):
        for given in (new_state, None):  # the saved state, and the forward launch made by the method itself
            A, Bu = env.vmap_linearize(state, action, given, rows=kind)
            torch.cuda.synchronize()
            assert env.last_linearize_launch == NAMES[kind]
            _check_shapes(env, A, Bu, want[kind][0].shape[1], (B,))
            dA, dB = rel_dist(_np(A), want[kind][0]), rel_dist(_np(Bu), want[kind][1])
            print(f"{env_name} dead={deadtime} {solver} B={B} control={control} rows={kind} new_state={'given' if given is not None else 'made'}: "
                  f"A {dA:.3e} Bu {dB:.3e} (|A| {np.abs(want[kind][0]).max():.3e}, |Bu| {np.abs(want[kind][1]).max():.3e})")
            assert dA <= 1e-8 and dB <= 1e-8


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_fp64_kernel_matches_the_twin(env_name, deadtime, solver):
    _fp64_vs_twin(env_name, deadtime, solver)


@pytest.mark.parametrize("deadtime", [0, 1])
def test_fp64_observation_rows_leave_out_the_reference_columns(deadtime):
    """PMSM with controlled currents: the observation has O + 2 columns, the Jacobian O rows (a reference column has no row, as it
    has no gradient anywhere else), and nothing else moves."""
    env, state, action, want, _, _ = _setup("pmsm", deadtime, "rk4", F64, control=("i_d", "i_q"))
    obs, _ = env.vmap_step(state, action)
    assert obs.shape[1] == want["obs"][0].shape[1] + 2
    _fp64_vs_twin("pmsm", deadtime, "rk4", control=("i_d", "i_q"))


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_fp32_kernel_within_32x_the_forward_floor(env_name, deadtime, solver):
    env, state, action, want, obs64, keep = _setup(env_name, deadtime, solver, torch.float32)
    excluded = 1.0 - keep.mean()
    assert excluded <= KINK_CAP
    obs, new_state = env.vmap_step(state, action)
    floor = obs_floor(_np(obs), obs64, env_name, keep)  # the fp32 forward launch, code this kernel does not touch
    bound = 32 * floor
    for kind in ("state", "obs"):
        A, Bu = env.vmap_linearize(state, action, new_state, rows=kind)
        torch.cuda.synchronize()
        _check_shapes(env, A, Bu, want[kind][0].shape[1], (B0,))
        dA, dB = rel_dist(_np(A), want[kind][0], keep), rel_dist(_np(Bu), want[kind][1], keep)
        print(f"{env_name} dead={deadtime} {solver} rows={kind}: forward floor {floor:.3e}, bound {bound:.3e}, A {dA:.3e} Bu {dB:.3e}, "
              f"excluded {excluded:.4f}")
        assert dA <= bound and dB <= bound


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_rows_are_what_the_step_kernel_returns_for_one_hot_cotangents(env_name, deadtime, solver):
    env, state, action, _, _, _ = _setup(env_name, deadtime, solver, F64)
    obs, new_state = env.vmap_step(state, action)
    S, O = env.physical_state_dim, obs.shape[1]
    one, zero = torch.ones(B0, dtype=F64, device=env.device), torch.zeros(B0, dtype=F64, device=env.device)
    for kind, R in (("state", S), ("obs", O)):
        A, Bu = env.vmap_linearize(state, action, new_state, rows=kind)
        a_rows, b_rows = [], []
        for r in range(R):
            if kind == "state":
                ga, gs = env.vmap_step_vjp(state, action, new_state, grad_state=[one if j == r else None for j in range(S)])
            else:
                e = torch.zeros(B0, O, dtype=F64, device=env.device)
                e[:, r] = 1.0
                ga, gs = env.vmap_step_vjp(state, action, new_state, grad_obs=e)
            a_rows.append(torch.stack([getattr(gs, n) for n in env.STATE_FIELDS], dim=-1))
            b_rows.append(ga)
        wa, wb = torch.stack(a_rows, dim=1), torch.stack(b_rows, dim=1)
        torch.cuda.synchronize()
        dA, dB = rel_dist(_np(A), _np(wa)), rel_dist(_np(Bu), _np(wb))
        print(f"{env_name} dead={deadtime} {solver} rows={kind}: A {dA:.3e} Bu {dB:.3e}, bit-equal {torch.equal(A, wa) and torch.equal(Bu, wb)}")
        assert float(wa.abs().max()) > 0
        assert dA <= 2e-8 and dB <= 2e-8


# ---------------------------------------------------------------------------------------------------------------- 4
def _trajectory(env_name, deadtime, solver, K, sub, lane_major, seed=41):
    spec = skewed_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B0, K, seed=seed)
    run = GpuRun(env_name, spec, F64, solver, "step", st, acts, sub=sub, lane_major_actions=lane_major)
    return run, spec


@pytest.mark.parametrize("lane_major", [True, False])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_trajectory_rows_equal_the_single_step_bit_for_bit(env_name, deadtime, solver, lane_major):
    K = 4
    run, spec = _trajectory(env_name, deadtime, solver, K, 1, lane_major)
    env, tau = run.env, spec["tau"]
    A_dim = env.action_dim
    assert (tuple(run.actions.stride()) == (1, A_dim * B0, B0)) == lane_major
    traj = _leaves(env, run.states)
    for kind in ("state", "obs"):
        A, Bu = env.vmap_linearize_ahead(run.states, run.actions, tau, tau, rows=kind)
        assert env.last_linearize_launch == NAMES[kind]
        R = env.physical_state_dim if kind == "state" else run.obs.shape[-1]
        _check_shapes(env, A, Bu, R, (B0, K))
        for n in range(K):
            a1, b1 = env.vmap_linearize([t[:, n] for t in traj], run.actions[:, n], [t[:, n + 1] for t in traj], rows=kind)
            torch.cuda.synchronize()
            same = torch.equal(A[:, n], a1) and torch.equal(Bu[:, n], b1)
            print(f"{env_name} dead={deadtime} {solver} lane_major={lane_major} rows={kind} n={n}: equal {same}, |A| {float(a1.abs().max()):.3e}")
            assert float(a1.abs().max()) > 0
            assert same


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", [c for c in CASES if c[0] != "pmsm"])
def test_substeps_against_the_trajectory_reverse_kernel(env_name, deadtime, solver):
    K, sub = 3, 2
    N = K * sub
    run, spec = _trajectory(env_name, deadtime, solver, K, sub, True, seed=43)
    env, tau = run.env, spec["tau"]
    S = env.physical_state_dim
    g_last = np.random.default_rng(44).normal(size=(B0, S))
    want_ga, want_gs = run.vjp(g_last=[g_last[:, j] for j in range(S)])
    A, Bu = env.vmap_linearize_ahead(run.states, run.actions, tau, tau * sub)
    _check_shapes(env, A, Bu, S, (B0, N))
    lam = dev(g_last, env)
    ga = torch.zeros(B0, K, env.action_dim, dtype=F64, device=env.device)
    for n in range(N - 1, -1, -1):
        ga[:, n // sub] += torch.einsum("bra,br->ba", Bu[:, n], lam)
        lam = torch.einsum("brs,br->bs", A[:, n], lam)
    torch.cuda.synchronize()
    d = [rel_dist(_np(ga), want_ga)] + [rel_dist(_np(lam[:, j]), want_gs[j]) for j in range(S)]
    print(f"{env_name} {solver}: action gradients {d[0]:.3e}, lambda_0 per leaf {[f'{x:.3e}' for x in d[1:]]}")
    assert float(np.abs(want_ga).max()) > 0
    assert max(d) <= 2e-8


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("B", [1, 63])
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "euler"), ("cartpole", None, "rk4"), ("pmsm", 1, "tsit5")])
def test_small_batches_hold_the_fp64_bound(env_name, deadtime, solver, B):
    _fp64_vs_twin(env_name, deadtime, solver, B=B)


def test_empty_batch_and_empty_trajectory_return_shaped_tensors_without_a_launch():
    env, _, _, _ = make_env("pmsm", 0, F64, "rk4")
    env.sim_ahead_semantics = "step"
    S, A_dim = env.physical_state_dim, env.action_dim
    empty = [torch.empty(0, dtype=F64, device=env.device) for _ in range(S)]
    for kind, R in (("state", S), ("obs", 8)):
        A, Bu = env.vmap_linearize(empty, torch.empty(0, A_dim, dtype=F64, device=env.device), empty, rows=kind)
        assert tuple(A.shape) == (0, R, S) and tuple(Bu.shape) == (0, R, A_dim)
        A, Bu = env.vmap_linearize_ahead([torch.empty(0, 4, dtype=F64, device=env.device) for _ in range(S)],
                                         torch.empty(0, 3, A_dim, dtype=F64, device=env.device), env.tau, env.tau, rows=kind)
        assert tuple(A.shape) == (0, 3, R, S) and tuple(Bu.shape) == (0, 3, R, A_dim)
    assert env.last_linearize_launch == ""
    env, _, _, _ = make_env("pendulum", B0, F64, "rk4")
    env.sim_ahead_semantics = "step"
    row0 = [torch.empty_strided((B0, 1), (1, B0), dtype=F64, device=env.device) for _ in range(2)]
    A, Bu = env.vmap_linearize_ahead(row0, torch.empty(B0, 0, 1, dtype=F64, device=env.device), env.tau, env.tau)
    assert tuple(A.shape) == (B0, 0, 2, 2) and tuple(Bu.shape) == (B0, 0, 2, 1) and A.grad_fn is None
    assert env.last_linearize_launch == ""


def test_an_action_slice_off_a_16_byte_boundary_is_accepted():
    env, state, action, want, _, _ = _setup("pmsm", 0, "rk4", F64)
    _, new_state = env.vmap_step(state, action)
    store = torch.empty(B0 * 2 + 1, dtype=F64, device=env.device)
    shifted = store[1:].view(B0, 2)
    shifted.copy_(action)
    assert shifted.data_ptr() % 16 == 8 and shifted.is_contiguous()
    A0, B0u = env.vmap_linearize(state, action, new_state)
    A1, B1u = env.vmap_linearize(state, shifted, new_state)
    torch.cuda.synchronize()
    assert torch.equal(A0, A1) and torch.equal(B0u, B1u)
    assert rel_dist(_np(A1), want["state"][0]) <= 1e-8 and rel_dist(_np(B1u), want["state"][1]) <= 1e-8


def test_outputs_carry_no_graph_whatever_the_inputs_and_the_switch_say():
    env, state, action, want, _, _ = _setup("cartpole", None, "rk4", F64)
    env.differentiable = True
    for n in env.STATE_FIELDS:
        getattr(state.physical_state, n).requires_grad_(True)
    action = action.clone().requires_grad_(True)
    with torch.enable_grad():
        A, Bu = env.vmap_linearize(state, action, rows="state")
        assert A.grad_fn is None and Bu.grad_fn is None and not A.requires_grad and not Bu.requires_grad
        obs, new_state = env.vmap_step(state, action)
        assert obs.grad_fn is not None  # the switch is on: the step itself records its node
        A2, Bu2 = env.vmap_linearize(state, action, new_state, rows="obs")
        assert A2.grad_fn is None and Bu2.grad_fn is None and not A2.requires_grad
    torch.cuda.synchronize()
    assert env.last_linearize_launch == NAMES["obs"]
    assert rel_dist(_np(A), want["state"][0]) <= 1e-8 and rel_dist(_np(A2), want["obs"][0]) <= 1e-8
    assert rel_dist(_np(Bu), want["state"][1]) <= 1e-8 and rel_dist(_np(Bu2), want["obs"][1]) <= 1e-8
