"""The reverse-mode kernel (sim_ahead_vjp_kernel) where tests/test_gpu_vjp.py does not reach: models off their (degenerate) default
parameters with asymmetric ranges, every wide instantiation, ragged batches, one and two action rows, substeps for every solver,
a solver step that is not the environment's tau, single-leaf and oddly laid-out cotangents, and the tank run dry.

The reference is the float64 torch twin (tests/helpers_vjp.py); tests/test_vjp_twin.py validates it against the fp64 CPU oracle
for each of these input families first and asserts, from the twin alone, every share of excluded environments used here.
The bounds are those of tests/test_gpu_vjp.py (derived there): fp64 kernel vs twin 1e-8 of each gradient tensor's largest
magnitude, directional finite difference 1e-6, fp32 kernel vs twin 32 x the fp32 forward's own distance from the twin on the same
inputs, environments within KINK_MARGIN of a kink excluded from the fp32 comparison only (at most KINK_CAP). None of them depends on
a parameter value or a shape, so none is new. Every case prints what it measured; the figures of an MI355X are in DESIGN.md §5."""
import numpy as np
import pytest
import torch

import oracle
from helpers import ANGLE_OBS, TRIG_FREE, circ_close, max_err, spec_of
from helpers_vjp import (CASES, DRY_MARGIN, DRY_STEP_FACTOR, KINK_CAP, KINK_MARGIN, SEM, SOLVERS, WIDE_CASES, WIDE_K, GpuRun, Twin,
                         case_spec, cotangents, dry_tank_inputs, obs_floor, rel_dist, skewed_spec, twin_grads, vjp_inputs,
                         wide_inputs)

pytestmark = pytest.mark.gpu

B0 = 256
F64 = torch.float64


def grad_dist(got, want, keep=None):
    """(grad_actions, grad leaves) of the kernel against the twin's: the largest relative distance over the tensors"""
    return max([rel_dist(got[0], want[0], keep)] + [rel_dist(g, w, keep) for g, w in zip(got[1], want[1])])


def fp64_vs_twin(env_name, spec, solver, semantics, st, acts, sub=1, step=None, groups=None, seed=5, **run_args):
    """One fp64 GPU run against the twin for the given cotangent groups (default: one group, everything) -> the run and the
    largest relative distance of each group"""
    run = GpuRun(env_name, spec, F64, solver, semantics, st, acts, sub=sub, step=step, **run_args)
    B, K = acts.shape[0], acts.shape[1]
    OW, S = run.obs.shape[-1], len(st)
    if groups is None:
        groups = [cotangents(np.random.default_rng(seed), B, K * sub + 1, OW, S)]
    tau = spec["tau"] if step is None else step
    want, _, _ = twin_grads(Twin(env_name, spec, solver, semantics), st, acts, tau, sub, groups, OW - len(run_args.get("control_state") or []))
    return run, [grad_dist(run.vjp(*grp), w) for grp, w in zip(groups, want)]


# ------------------------------------------------------------------------------------------------- A: off-default, asymmetric models
@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_skewed_fp64_kernel_matches_the_twin_and_its_forward_the_oracle(env_name, deadtime, solver, semantics):
    """Forward bound: the one tests/test_gpu_parity.py uses for fp64 trajectories (identical bits for the models without sin / cos,
    1e-9 relative + absolute on normalised observations, wrapped angles on the circle, for the others)."""
    spec = skewed_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B0, 24, seed=71)
    run, (d,) = fp64_vs_twin(env_name, spec, solver, semantics, st, acts)
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B0)
    o_ref, _, _ = oracle.sim_ahead(env_name, solver, st, acts, props, spec["tau"], env_tau=spec["tau"], semantics=SEM[semantics])
    obs = run.obs.cpu().numpy()
    print(f"skewed {env_name} dead={deadtime} {solver} {semantics}: gradients rel dist {d:.3e}, forward vs oracle max |d obs| "
          f"{max_err(obs, o_ref):.3e}")
    assert d <= 1e-8
    if env_name in TRIG_FREE:
        assert np.array_equal(obs, np.asarray(o_ref))
    else:
        assert circ_close(obs, o_ref, ANGLE_OBS.get(env_name, []), 1e-9, 1e-9)


def fp32_vs_twin(env_name, spec, solver, semantics, st32, acts32, sub=1, seed=5, **run_args):
    """One fp32 GPU run against the twin on the same (fp32-representable) values -> run, forward floor, gradient distance over the
    kept environments, excluded share"""
    st, acts = [v.astype(np.float64) for v in st32], acts32.astype(np.float64)
    run = GpuRun(env_name, spec, torch.float32, solver, semantics, st32, acts32, sub=sub, **run_args)
    B, K = acts.shape[0], acts.shape[1]
    S, O = len(st), run.obs.shape[-1]
    grp = cotangents(np.random.default_rng(seed), B, K * sub + 1, O, S)
    r32 = lambda g: g.astype(np.float32).astype(np.float64)
    grp = (r32(grp[0]), [r32(g) for g in grp[1]], [r32(g) for g in grp[2]])
    (want,), kd, obs64 = twin_grads(Twin(env_name, spec, solver, semantics), st, acts, spec["tau"], sub, [grp], O)
    keep = np.ones(B, dtype=bool) if kd is None else (kd.numpy() >= KINK_MARGIN)
    floor = obs_floor(run.obs.cpu().numpy(), obs64, env_name, keep)
    got = run.vjp(*grp)
    return run, floor, grad_dist(got, want, keep), 1.0 - keep.mean(), got


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_skewed_fp32_kernel_within_32x_the_forward_floor(env_name, deadtime, solver, semantics):
    spec = skewed_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B0, 24, seed=71, np_dtype=np.float32)
    _, floor, d, excluded, _ = fp32_vs_twin(env_name, spec, solver, semantics, st, acts)
    print(f"skewed {env_name} dead={deadtime} {solver} {semantics}: forward floor {floor:.3e}, bound {32 * floor:.3e}, gradients {d:.3e}, "
          f"excluded {excluded:.4f}")
    assert excluded <= KINK_CAP
    assert d <= 32 * floor


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_skewed_directional_finite_difference_of_the_fp64_forward(env_name, deadtime, semantics):
    """Independent of the twin: <grad_actions, delta> per environment against the central difference (h = 1e-5) of two fp64 forward
    launches at the skewed spec, Tsit5. The tank steps by 100 tau, for the reason
    test_gpu_vjp.test_directional_finite_difference_of_the_fp64_forward gives (at tau its level hardly moves and the difference
    quotient's own round-off exceeds the bound)."""
    solver = "tsit5"
    spec = skewed_spec(env_name, deadtime)
    step = 100 * spec["tau"] if env_name == "fluid_tank" else None
    K = 24
    st, acts = vjp_inputs(env_name, spec, B0, K, seed=71)
    rng = np.random.default_rng(8)
    delta = rng.normal(size=acts.shape)
    h = 1e-5
    run = GpuRun(env_name, spec, F64, solver, semantics, st, acts, step=step)
    w_obs, w_states, w_last = cotangents(rng, B0, K + 1, run.obs.shape[-1], len(st))

    def loss(r):  # per environment
        L = (r.obs.cpu().numpy() * w_obs).sum(axis=(1, 2))
        for n, ws, wl in zip(r.env.STATE_FIELDS, w_states, w_last):
            L = L + (getattr(r.states.physical_state, n).cpu().numpy() * ws).sum(axis=1)
            L = L + getattr(r.last.physical_state, n).cpu().numpy() * wl
        return L

    ga, _ = run.vjp(w_obs, w_states, w_last)
    lp = loss(GpuRun(env_name, spec, F64, solver, semantics, st, acts + h * delta, step=step))
    lm = loss(GpuRun(env_name, spec, F64, solver, semantics, st, acts - h * delta, step=step))
    fd = (lp - lm) / (2 * h)
    scale = float(np.max(np.abs(fd)))
    err = float(np.max(np.abs((ga * delta).sum(axis=(1, 2)) - fd))) / scale
    print(f"skewed {env_name} dead={deadtime} {solver} {semantics}: directional derivative rel err {err:.3e} (scale {scale:.3e})")
    assert err <= 1e-6


# ------------------------------------------------------------------------------------------------- B: every wide instantiation
def flat(got):
    return np.concatenate([got[0].ravel()] + list(got[1]))


@pytest.mark.parametrize("env_name,elem,solver,semantics", WIDE_CASES)
def test_every_wide_instantiation_matches_the_twin_and_the_narrow_form(env_name, elem, solver, semantics):
    """16 bytes per lane forced, B = V * 326 (one full workgroup, one full wavefront and six lanes of a third; B % 64 != 0),
    K = 7, substeps 3 (PMSM: 1): the twin bound of the number format, and the bits of the V = 1 run of the same inputs."""
    spec = spec_of(env_name)
    V, sub, st, acts = wide_inputs(env_name, elem, spec)
    B = V * 326
    assert acts.shape[0] == B and B % 64 != 0
    if elem == 8:
        grp = cotangents(np.random.default_rng(5), B, WIDE_K * sub + 1, len(st) if env_name != "pmsm" else 8, len(st))
        run, (d,) = fp64_vs_twin(env_name, spec, solver, semantics, st, acts, sub=sub, groups=[grp], envs_per_lane=V)
        got = run.vjp(*grp)
        narrow = GpuRun(env_name, spec, F64, solver, semantics, st, acts, sub=sub, envs_per_lane=1)
        ref = narrow.vjp(*grp)
        bound = 1e-8
        note = ""
    else:
        run, floor, d, excluded, got = fp32_vs_twin(env_name, spec, solver, semantics, st, acts, sub=sub, envs_per_lane=V)
        narrow, _, _, _, ref = fp32_vs_twin(env_name, spec, solver, semantics, st, acts, sub=sub, envs_per_lane=1)
        bound = 32 * floor
        note = f", forward floor {floor:.3e}, excluded {excluded:.4f}"
        assert excluded <= KINK_CAP
    same = np.array_equal(flat(got), flat(ref))
    print(f"wide {env_name} fp{8 * elem} {solver} {semantics}: {run.launch}, B={B}, substeps={sub}, gradients {d:.3e}, bound {bound:.3e}"
          f"{note}, same bits as V=1: {same}")
    assert run.launch == f"sim_ahead_vjp_kernel (V={V})"
    assert narrow.launch == "sim_ahead_vjp_kernel (V=1)"
    assert np.isfinite(flat(got)).all() and np.abs(flat(got)).max() > 0
    assert d <= bound
    assert same


def test_wide_form_with_a_control_state_column():
    """OW = O + n_control is the row stride of the observation cotangent: 16-byte loads at that stride, ragged batch"""
    from exciting_environments_amd import _native

    env_name, solver, semantics, V = "pendulum", "tsit5", "ahead", 2
    spec = spec_of(env_name)
    B, K = V * 326, WIDE_K
    st, acts = vjp_inputs(env_name, spec, B, K, seed=72)
    run = GpuRun(env_name, spec, F64, solver, semantics, st, acts, control_state=["theta"], reference={"theta": np.full(B, 0.3)})
    assert run.obs.shape[-1] == 3
    grp = cotangents(np.random.default_rng(7), B, K + 1, 3, len(st))
    (want,), _, _ = twin_grads(Twin(env_name, spec, solver, semantics), st, acts, spec["tau"], 1, [grp], 2)
    narrow = run.vjp(*grp)
    assert run.launch == "sim_ahead_vjp_kernel (V=1)"
    run.env.launch_opts = _native.launch_opts(envs_per_lane=V)
    got = run.vjp(*grp)
    d = grad_dist(got, want)
    print(f"wide pendulum control_state=['theta']: {run.launch}, gradients {d:.3e}")
    assert run.launch == f"sim_ahead_vjp_kernel (V={V})"
    assert d <= 1e-8
    assert np.array_equal(flat(got), flat(narrow))


def test_wide_form_with_row_major_actions_at_a_ragged_batch():
    """Row-major [B, K, A] actions are transposed into the workspace first: two action components, B % 64 != 0"""
    env_name, solver, semantics, V = "pmsm", "euler", "ahead", 4
    spec = spec_of(env_name)
    _, sub, st, acts = wide_inputs(env_name, 4, spec)
    run, floor, d, excluded, got = fp32_vs_twin(env_name, spec, solver, semantics, st, acts, envs_per_lane=V, lane_major_actions=False)
    assert tuple(run.actions.stride()) == (acts.shape[1] * 2, 2, 1)
    lane, _, _, _, ref = fp32_vs_twin(env_name, spec, solver, semantics, st, acts, envs_per_lane=V)
    print(f"wide pmsm euler fp32 row-major actions: {run.launch}, forward floor {floor:.3e}, gradients {d:.3e}, excluded {excluded:.4f}")
    assert run.launch == lane.launch == f"sim_ahead_vjp_kernel (V={V})"
    assert excluded <= KINK_CAP and d <= 32 * floor
    assert np.array_equal(flat(got), flat(ref))


# ------------------------------------------------------------------------------------------------- C: batch tails
TAIL_COMBOS = [("pendulum", None, "tsit5", "ahead"), ("cartpole", None, "euler", "step"), ("pmsm", 1, "rk4", "ahead")]


@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("env_name,deadtime,solver,semantics", TAIL_COMBOS)
def test_batch_tails_at_one_environment_per_lane(env_name, deadtime, solver, semantics, B):
    spec = case_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B, 6, seed=73)
    for lane_major in (True, False):
        run, (d,) = fp64_vs_twin(env_name, spec, solver, semantics, st, acts, lane_major_actions=lane_major)
        print(f"tail {env_name} {solver} {semantics} B={B} {'lane' if lane_major else 'row'}-major actions: {run.launch}, rel dist {d:.3e}")
        assert run.launch == "sim_ahead_vjp_kernel (V=1)"
        assert d <= 1e-8


def test_a_forced_wide_form_at_an_indivisible_batch_is_refused():
    from exciting_environments_amd import _native

    spec = spec_of("pendulum")
    B, K = 63, 6
    st, acts = vjp_inputs("pendulum", spec, B, K, seed=73)
    run = GpuRun("pendulum", spec, F64, "tsit5", "ahead", st, acts)
    grp = cotangents(np.random.default_rng(5), B, K + 1, 2, 2)
    run.env.launch_opts = _native.launch_opts(envs_per_lane=2)
    with pytest.raises(RuntimeError, match=r"envs_per_lane = 2 is not available"):
        run.vjp(*grp)
    run.env.launch_opts = _native.launch_opts(envs_per_lane=1)
    run.vjp(*grp)
    assert run.launch == "sim_ahead_vjp_kernel (V=1)"


@pytest.mark.parametrize("B,V", [((1 << 17) + 1, 1), (1 << 17, 2)])
def test_large_batch_falls_back_to_one_per_lane_when_indivisible(B, V):
    """The automatic form: two fp64 environments per lane from B = 2^17 on, one when B is odd; the last 512 environments
    (the partial last workgroup at 2^17 + 1) against the twin"""
    env_name, solver, semantics, K, NS = "mass_spring_damper", "euler", "ahead", 2, 512
    spec = spec_of(env_name)
    st, acts = vjp_inputs(env_name, spec, B, K, seed=73)
    run = GpuRun(env_name, spec, F64, solver, semantics, st, acts)
    rng = np.random.default_rng(10)
    g_obs, g_last = rng.normal(size=(B, K + 1, 2)), [rng.normal(size=B) for _ in range(2)]
    ga, gs = run.vjp(g_obs, None, g_last)
    sl = slice(B - NS, B)
    (want,), _, _ = twin_grads(Twin(env_name, spec, solver, semantics), [v[sl] for v in st], acts[sl], spec["tau"], 1,
                               [(g_obs[sl], None, [g[sl] for g in g_last])], 2)
    d = grad_dist((ga[sl], [g[sl] for g in gs]), want)
    print(f"mass_spring_damper euler fp64 B={B}: {run.launch}, last {NS} environments rel dist {d:.3e}")
    assert run.launch == f"sim_ahead_vjp_kernel (V={V})"
    assert np.isfinite(ga).all() and d <= 1e-8


# ------------------------------------------------------------------------------------------------- D: step bookkeeping
@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_one_and_two_action_rows_pendulum(solver, semantics):
    """K = 1: the prologue loads row K - 1 twice and no step has a next row; K = 2: one step with, one without"""
    spec = spec_of("pendulum")
    for K in (1, 2):
        st, acts = vjp_inputs("pendulum", spec, B0, K, seed=74)
        for sub in (1, 3):
            _, (d,) = fp64_vs_twin("pendulum", spec, solver, semantics, st, acts, sub=sub)
            print(f"pendulum {solver} {semantics} K={K} substeps={sub}: rel dist {d:.3e}")
            assert d <= 1e-8


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("deadtime", [0, 1])
def test_one_and_two_action_rows_pmsm(deadtime, solver, semantics):
    """K = 1 under "ahead": the linspace of the predicted angles has one point (K - 1 = 0 as its divisor)"""
    spec = case_spec("pmsm", deadtime)
    for K in (1, 2):
        st, acts = vjp_inputs("pmsm", spec, B0, K, seed=74)
        _, (d,) = fp64_vs_twin("pmsm", spec, solver, semantics, st, acts)
        print(f"pmsm dead={deadtime} {solver} {semantics} K={K}: rel dist {d:.3e}")
        assert d <= 1e-8


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name", ["mass_spring_damper", "cartpole"])
def test_three_substeps_for_every_solver_and_semantics(env_name, solver, semantics):
    spec = spec_of(env_name)
    st, acts = vjp_inputs(env_name, spec, B0, 5, seed=74)
    _, (d,) = fp64_vs_twin(env_name, spec, solver, semantics, st, acts, sub=3)
    print(f"{env_name} {solver} {semantics} K=5 substeps=3: rel dist {d:.3e}")
    assert d <= 1e-8


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("pmsm", 0, "rk4"), ("pmsm", 1, "rk4")])
def test_a_solver_step_of_half_the_environment_tau(env_name, deadtime, solver, semantics):
    """obs_stepsize = action_stepsize = tau / 2: the kernel's dt and env_tau differ (PMSM's angle prediction and the times of its
    "ahead" clips use the second). The twin is built with the environment's tau and steps by tau / 2."""
    spec = case_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B0, 24, seed=74)
    _, (d,) = fp64_vs_twin(env_name, spec, solver, semantics, st, acts, step=0.5 * spec["tau"])
    print(f"{env_name} dead={deadtime} {solver} {semantics} step = tau / 2: rel dist {d:.3e}")
    assert d <= 1e-8


# ------------------------------------------------------------------------------------------------- E: sparse / oddly laid-out cotangents
SPARSE = [("pendulum", "tsit5", "ahead", [1], [0]), ("pmsm", "rk4", "ahead", [5, 0], [4]), ("pmsm", "euler", "step", [5, 0], [5])]


@pytest.mark.parametrize("env_name,solver,semantics,state_leaves,last_leaves", SPARSE)
def test_single_leaf_cotangents(env_name, solver, semantics, state_leaves, last_leaves):
    """Per-leaf None: a single state-trajectory leaf next to the observation cotangent and alone, a single last-state leaf.
    PMSM: leaf 5 is the torque (its cotangent reaches the currents through post_vjp), leaf 0 u_d_buffer."""
    spec = spec_of(env_name)
    K = 12
    st, acts = vjp_inputs(env_name, spec, B0, K, seed=75)
    S = len(st)
    g_obs, g_states, g_last = cotangents(np.random.default_rng(5), B0, K + 1, 2 if env_name == "pendulum" else 8, S)
    only = lambda gs, j: [g if q == j else None for q, g in enumerate(gs)]
    groups, names = [], []
    for j in state_leaves:
        groups += [(g_obs, only(g_states, j), None), (None, only(g_states, j), None)]
        names += [f"observations + state leaf {j}", f"state leaf {j} alone"]
    for j in last_leaves:
        groups.append((None, None, only(g_last, j)))
        names.append(f"last-state leaf {j} alone")
    _, ds = fp64_vs_twin(env_name, spec, solver, semantics, st, acts, groups=groups)
    for name, d in zip(names, ds):
        print(f"{env_name} {solver} {semantics} {name}: rel dist {d:.3e}")
    assert max(ds) <= 1e-8


@pytest.mark.parametrize("env_name,solver", [("pendulum", "tsit5"), ("pmsm", "rk4")])
def test_layouts_of_one_observation_cotangent_give_the_same_bits(env_name, solver):
    """Lane-major as the kernel reads it, contiguous row-major, a lane-major view whose data pointer is not 16-byte aligned (the copy
    path of _lane_major), and an expanded scalar against its materialised lane-major form"""
    spec = spec_of(env_name)
    K = 12
    st, acts = vjp_inputs(env_name, spec, B0, K, seed=75)
    run = GpuRun(env_name, spec, F64, solver, "ahead", st, acts)
    env, OW = run.env, run.obs.shape[-1]
    shape, strides = (B0, K + 1, OW), (1, OW * B0, B0)
    values = torch.as_tensor(np.random.default_rng(5).normal(size=shape), dtype=F64, device=env.device)
    lane = torch.empty_strided(shape, strides, dtype=F64, device=env.device)
    lane.copy_(values)
    row = values.contiguous()
    store = torch.empty(lane.numel() + 1, dtype=F64, device=env.device)
    shifted = store.as_strided(shape, strides, 1)
    shifted.copy_(values)
    assert tuple(row.stride()) == ((K + 1) * OW, OW, 1) and lane.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 8
    ref = flat(run.vjp(lane))
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    assert np.array_equal(ref, flat(run.vjp(row)))
    assert np.array_equal(ref, flat(run.vjp(shifted)))
    scalar = torch.tensor(0.37, dtype=F64, device=env.device).expand(shape)
    full = torch.empty_strided(shape, strides, dtype=F64, device=env.device)
    full.fill_(0.37)
    assert tuple(scalar.stride()) == (0, 0, 0)
    assert np.array_equal(flat(run.vjp(full)), flat(run.vjp(scalar)))
    (want,), _, _ = twin_grads(Twin(env_name, spec, solver, "ahead"), st, acts, spec["tau"], 1, [(values.cpu().numpy(), None, None)], OW)
    d = grad_dist(run.vjp(shifted), want)
    print(f"{env_name} {solver} misaligned lane-major observation cotangent: rel dist {d:.3e}")
    assert d <= 1e-8


# ------------------------------------------------------------------------------------------------- F: the dry tank
@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_dry_tank(solver, semantics):
    """The subgradient convention at h <= 0 (derivative 0 in f_vjp and post_vjp) where it acts: 10 ... 22 % of the saved rows are
    exactly dry (tests/test_vjp_twin.py). fp64 only, no finite difference (a difference quotient across the kink is meaningless, and
    the fp32 margin would exclude most of this regime). Environments in which the twin reads a NONZERO level within DRY_MARGIN of
    the range from 0 are excluded (at most KINK_CAP, asserted on the CPU; none with these inputs). Besides the twin bound: the
    gradient entries that are exactly 0 are the same on both sides, and the wide form gives the bits of the narrow one here too.
    This test found the RK solvers under "ahead" wrong by 5e-2 (Tsit5) and 2.7e-1 (RK4) of the largest gradient: the saved rows
    hold max(h, 0), and a stage state built from a clamped row is not the one the forward built from the raw level below 0. The
    reverse call now restores the raw levels first (vjp_raw_rows_kernel)."""
    spec = spec_of("fluid_tank")
    st, acts = dry_tank_inputs()
    B, K = acts.shape[0], acts.shape[1]
    step = DRY_STEP_FACTOR * spec["tau"]
    run = GpuRun("fluid_tank", spec, F64, solver, semantics, st, acts, step=step)
    g_obs, g_states, g_last = cotangents(np.random.default_rng(5), B, K + 1, 1, 1)
    groups = [(g_obs, g_states, g_last), (None, None, g_last)]
    twin = Twin("fluid_tank", spec, solver, semantics)
    want, _, _ = twin_grads(twin, st, acts, step, 1, groups, 1)
    keep = ~twin.near_dry(DRY_MARGIN).numpy()
    assert 1.0 - keep.mean() <= KINK_CAP
    dry = float((run.states.physical_state.height == 0).double().mean())
    worst, zeros_agree = 0.0, True
    for grp, w, name in zip(groups, want, ("everything", "last_state only")):
        got = run.vjp(*grp)
        d = grad_dist(got, w, keep)
        zg, zw = flat(got) == 0, flat(w) == 0
        keep_flat = np.concatenate([np.repeat(keep, K), keep])
        same = bool(np.array_equal(zg[keep_flat], zw[keep_flat]))
        print(f"dry tank {solver} {semantics} {name}: {dry:.3f} of the saved rows dry, rel dist {d:.3e}, exact zeros: twin "
              f"{zw[keep_flat].mean():.3f} kernel {zg[keep_flat].mean():.3f} of the entries, same set: {same}")
        worst, zeros_agree = max(worst, d), zeros_agree and same
    assert dry >= 0.05
    assert worst <= 1e-8
    assert zeros_agree
    wide = GpuRun("fluid_tank", spec, F64, solver, semantics, st, acts, step=step, envs_per_lane=2)
    got2 = wide.vjp(*groups[0])
    assert wide.launch == "sim_ahead_vjp_kernel (V=2)"
    assert np.array_equal(flat(got2), flat(run.vjp(*groups[0])))
