"""Parity of the HIP kernels (through the Python mirror -> C ABI) against the reference's golden fixtures and
the fixture-pinned CPU oracle. Everything here needs an MI355X: run with ``-m gpu``.

Tolerances (stated per regime, SURVEY.md §7 "Tolerance must be stated per regime"):
  * fp64 kernel vs the reference fixtures: the reference's own ``allclose(rtol=1e-16 | 1e-8, atol=1e-8)``.
  * trig-free environments (mass-spring-damper, fluid tank), any dtype, any solver: BIT-EXACT vs the oracle.
  * environments with sin/cos: fp64 <= 1e-9, fp32 <= 1e-5 relative (+ the same absolute floor on O(1) normalised
    observations), short horizons so chaotic amplification does not mask a real bug.
"""
import numpy as np
import pytest
import torch

import oracle
from conftest import ENV_NAMES, golden_rtol
from helpers import (ANGLE_OBS, ANGLE_STATES, NP_DTYPE, TRIG_FREE, circ_close, make_env, max_err, phys_np,
                     random_state, spec_of, to_state)

pytestmark = pytest.mark.gpu

SOLVERS = ["euler", "rk4", "tsit5"]


def _tol(env, dtype):
    if env in TRIG_FREE:
        return 0.0, 0.0
    return (1e-9, 1e-9) if dtype == torch.float64 else (1e-5, 1e-5)


def _close(env, got, want, dtype, obs_cols=True):
    rtol, atol = _tol(env, dtype)
    if rtol == 0.0:
        return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)
    cols = ANGLE_OBS.get(env, []) if obs_cols else []
    return circ_close(got, want, cols, rtol, atol)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_fixture_step_path_fp64(env_name, golden):
    """The reference's test_step_results on the GPU: K launches of vmap_step, fp64, Euler, B replicas."""
    g = golden[env_name]
    B = 64
    env, props, keep, spec = make_env(env_name, B, torch.float64)
    obs0 = torch.as_tensor(np.repeat(g["observations"][:1], B, axis=0), device=env.device)
    state = env.vmap_generate_state_from_observation(obs0)
    acts = torch.as_tensor(g["actions"], dtype=torch.float64, device=env.device)
    gen = [obs0]
    for k in range(acts.shape[0]):
        obs, state = env.vmap_step(state, acts[k].expand(B, -1))
        gen.append(obs)
    gen = torch.stack(gen, dim=1).cpu().numpy()
    for b in (0, B - 1):
        assert np.allclose(gen[b], g["observations"], rtol=golden_rtol(env_name), atol=1e-8)
    assert np.array_equal(gen, np.repeat(gen[:1], B, axis=0))


@pytest.mark.parametrize("layout", ["lane_major", "env_major"])
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_fixture_sim_ahead_fp64(env_name, layout, golden):
    """One persistent launch over the whole fixture (10 000 steps; PMSM 1 000), SEM_STEP: reproduces the fixture
    and is bit-identical to K vmap_step launches."""
    g = golden[env_name]
    B = 8
    env, props, keep, spec = make_env(env_name, B, torch.float64)
    env.sim_ahead_semantics = "step"
    env.traj_layout = layout
    obs0 = torch.as_tensor(np.repeat(g["observations"][:1], B, axis=0), device=env.device)
    state = env.vmap_generate_state_from_observation(obs0)
    acts = torch.as_tensor(np.repeat(g["actions"][None], B, axis=0), device=env.device)
    obs, states, last = env.vmap_sim_ahead(state, acts, env.tau, env.tau)
    got = obs.cpu().numpy()
    assert got.shape == (B,) + g["observations"].shape
    assert np.allclose(got[0][1:], g["observations"][1:], rtol=golden_rtol(env_name), atol=1e-8)
    assert np.array_equal(got, np.repeat(got[:1], B, axis=0))
    s = state
    for k in range(200):
        o, s = env.vmap_step(s, acts[:, k])
        assert torch.equal(o, obs[:, k + 1]), f"step {k}"
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(last.physical_state, n), getattr(states.physical_state, n)[:, -1])


# fp32 kernels against the reference-held fixtures (fp64 Euler trajectories): the north-star's "<= 1e-5 relative vs the
# reference" as an assertion on reference data. Observations are normalised to [-1, 1], so the error is measured in units of
# each signal's full scale (angles on the circle). Horizons: the first 100 steps at 1e-5 for all six environments
# (measured: <= 4.6e-6, PMSM the largest), the first 1000 steps at 1e-4 for the five whose fixture stays bounded
# (measured <= 1.7e-5; the PMSM fixture starts at the default 1728 rad/s, where explicit Euler at tau = 1e-4 is unstable
# — SURVEY.md §0 — so fp32 and fp64 separate exponentially there).
FP32_FIXTURE_HORIZONS = ((100, 1e-5), (1000, 1e-4))


def _fixture_err(env_name, got, want):
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    for c in ANGLE_OBS.get(env_name, []):
        d[..., c] = np.minimum(d[..., c], np.abs(2.0 - d[..., c]))
    return d


# The WHOLE fixture (10 000 steps) in fp32, one launch, against the reference's fp64 data — for the systems whose own fp32-vs-fp64
# separation permits a bound (the fp32 CPU oracle against the same fixtures, full length: mass-spring-damper 1.1e-7, fluid tank
# 3.9e-6, cart-pole 4.5e-6, pendulum 4.6e-5, acrobot 1.5e-3 — the double pendulum amplifies rounding; the PMSM fixture is
# unstable for explicit Euler, see above). Tolerance: 1e-5 where that floor is below it, else a stated multiple of the floor.
FP32_FIXTURE_FULL_LENGTH = {"mass_spring_damper": 1e-5, "fluid_tank": 1e-5, "cartpole": 1e-5, "pendulum": 1e-4, "acrobot": 1e-2}


@pytest.mark.parametrize("semantics", ["step", "ahead"])
@pytest.mark.parametrize("env_name", sorted(FP32_FIXTURE_FULL_LENGTH))
def test_fixture_fp32_whole_fixture(env_name, semantics, golden):
    g = golden[env_name]
    B = 8
    env, props, keep, spec = make_env(env_name, B, torch.float32)
    env.sim_ahead_semantics = semantics
    obs0 = torch.as_tensor(np.repeat(g["observations"][:1], B, axis=0), dtype=torch.float32, device=env.device)
    state = env.vmap_generate_state_from_observation(obs0)
    acts = torch.as_tensor(np.repeat(g["actions"][None], B, axis=0), dtype=torch.float32, device=env.device)
    obs, states, last = env.vmap_sim_ahead(state, acts, env.tau, env.tau)
    got = obs.cpu().numpy()
    assert got.shape == (B,) + g["observations"].shape
    err = _fixture_err(env_name, got[0], g["observations"])
    assert err.max() <= FP32_FIXTURE_FULL_LENGTH[env_name], (env_name, semantics, err.max())


@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_fixture_fp32_step_path(env_name, golden):
    """fp32 vmap_step launches against the reference's fp64 fixture."""
    g = golden[env_name]
    B = 32
    env, props, keep, spec = make_env(env_name, B, torch.float32)
    obs0 = torch.as_tensor(np.repeat(g["observations"][:1], B, axis=0), dtype=torch.float32, device=env.device)
    state = env.vmap_generate_state_from_observation(obs0)
    horizon = 100 if env_name == "pmsm" else 1000
    acts = torch.as_tensor(g["actions"][:horizon], dtype=torch.float32, device=env.device)
    rows = [obs0]
    for k in range(horizon):
        obs, state = env.vmap_step(state, acts[k].expand(B, -1))
        rows.append(obs)
    got = torch.stack(rows, dim=1).cpu().numpy()
    assert np.array_equal(got, np.repeat(got[:1], B, axis=0))
    err = _fixture_err(env_name, got[0], g["observations"][:horizon + 1])
    for n, tol in FP32_FIXTURE_HORIZONS:
        if n <= horizon:
            assert err[:n + 1].max() <= tol, (env_name, n, err[:n + 1].max())


@pytest.mark.parametrize("semantics", ["step", "ahead"])
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_fixture_fp32_sim_ahead(env_name, semantics, golden):
    """fp32 vmap_sim_ahead (one persistent launch, both semantics) against the reference's fp64 fixture."""
    g = golden[env_name]
    B = 8
    env, props, keep, spec = make_env(env_name, B, torch.float32)
    env.sim_ahead_semantics = semantics
    obs0 = torch.as_tensor(np.repeat(g["observations"][:1], B, axis=0), dtype=torch.float32, device=env.device)
    state = env.vmap_generate_state_from_observation(obs0)
    horizon = 100 if env_name == "pmsm" else 1000
    acts = torch.as_tensor(np.repeat(g["actions"][None, :horizon], B, axis=0), dtype=torch.float32, device=env.device)
    obs, states, last = env.vmap_sim_ahead(state, acts, env.tau, env.tau)
    got = obs.cpu().numpy()
    assert np.array_equal(got, np.repeat(got[:1], B, axis=0))
    err = _fixture_err(env_name, got[0], g["observations"][:horizon + 1])
    for n, tol in FP32_FIXTURE_HORIZONS:
        if n <= horizon:
            assert err[:n + 1].max() <= tol, (env_name, semantics, n, err[:n + 1].max())


# ------------------------------------------------------------------------------------------------ vs oracle
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_vmap_step_matches_oracle(env_name, solver, dtype):
    B = 4096 + 37  # ragged: not a multiple of the workgroup size
    env, props, keep, spec = make_env(env_name, B, dtype, solver)
    st = random_state(env_name, B, NP_DTYPE[dtype], spec, seed=11)
    rng = np.random.default_rng(12)
    act = rng.uniform(-1.2, 1.2, (B, env.action_dim)).astype(NP_DTYPE[dtype])
    obs, new = env.vmap_step(to_state(env, st), torch.as_tensor(act, device=env.device))
    o_ref, s_ref = oracle.step(env_name, solver, st, act, props, spec["tau"])
    assert obs.shape == o_ref.shape
    assert _close(env_name, obs.cpu().numpy(), o_ref, dtype), max_err(obs.cpu().numpy(), o_ref)
    got = phys_np(env, new)
    rtol, atol = _tol(env_name, dtype)
    for j, n in enumerate(env.STATE_FIELDS):
        scale = max(1.0, float(np.abs(s_ref[j]).max()))
        if rtol == 0:
            assert np.array_equal(got[j], s_ref[j]), n
        elif j in ANGLE_STATES.get(env_name, []):
            assert circ_close(got[j][:, None], s_ref[j][:, None], [0], rtol, atol * scale, period=2 * np.pi), n
        else:
            assert np.allclose(got[j], s_ref[j], rtol=rtol, atol=atol * scale), (n, max_err(got[j], s_ref[j]))
    assert bool(new.additions.active_solver_state.all())


@pytest.mark.parametrize("semantics", ["step", "ahead"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_vmap_sim_ahead_matches_oracle(env_name, solver, dtype, semantics):
    """The lean lane-major kernel at ONE environment per lane (what the batch rule gives B = 2048), K = 64. The wider lanes of every
    instantiation are held against this form and the oracle in tests/test_gpu_lean_forms.py."""
    from exciting_environments_amd import _native

    B, K = 2048, 64
    env, props, keep, spec = make_env(env_name, B, dtype, solver)
    env.sim_ahead_semantics = semantics
    st = random_state(env_name, B, NP_DTYPE[dtype], spec, seed=21)
    rng = np.random.default_rng(22)
    acts = rng.uniform(-1, 1, (B, K, env.action_dim)).astype(NP_DTYPE[dtype])
    a_dev = env.new_actions_buffer(K)
    a_dev.copy_(torch.as_tensor(acts, device=env.device))
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), a_dev, env.tau, env.tau)
    assert _native.last_launch() == "sim_ahead_kernel (V=1)", _native.last_launch()
    sem = oracle.SEM_STEP if semantics == "step" else oracle.SEM_AHEAD
    o_ref, s_ref, l_ref = oracle.sim_ahead(env_name, solver, st, acts, props, spec["tau"], semantics=sem)
    assert tuple(obs.shape) == o_ref.shape
    assert _close(env_name, obs.cpu().numpy(), o_ref, dtype), max_err(obs.cpu().numpy(), o_ref)
    rtol, atol = _tol(env_name, dtype)
    for j, n in enumerate(env.STATE_FIELDS):
        got = getattr(states.physical_state, n).cpu().numpy()
        got_last = getattr(last.physical_state, n).cpu().numpy()
        assert np.array_equal(got[:, -1], got_last)
        scale = max(1.0, float(np.nanmax(np.abs(s_ref[j]))))
        if rtol == 0:
            assert np.array_equal(got, s_ref[j]), n
        elif j in ANGLE_STATES.get(env_name, []):
            assert circ_close(got[..., None], s_ref[j][..., None], [0], rtol, atol * scale, period=2 * np.pi), n
        else:
            assert np.allclose(got, s_ref[j], rtol=rtol, atol=atol * scale), (n, max_err(got, s_ref[j]))


@pytest.mark.parametrize("vec", [1, 2, 4])
@pytest.mark.parametrize("env_name", ["pmsm", "pendulum", "mass_spring_damper"])
def test_envs_per_lane_variants_are_bit_identical(env_name, vec):
    """V = 1 / 2 / 4 environments per lane and the env-major (reference row-major) layout give identical bits."""
    from exciting_environments_amd import _native

    B, K = 1024, 33
    env, props, keep, spec = make_env(env_name, B, torch.float32)
    st = random_state(env_name, B, np.float32, spec, seed=31)
    acts = np.random.default_rng(32).uniform(-1, 1, (B, K, env.action_dim)).astype(np.float32)
    a_lane = env.new_actions_buffer(K)
    a_lane.copy_(torch.as_tensor(acts, device=env.device))
    a_env = torch.as_tensor(acts, device=env.device)
    env.traj_layout = "env_major"
    env.env_major_fused, env.env_major_workspace = False, False  # generic-stride kernel path
    ref_obs, ref_states, ref_last = env.vmap_sim_ahead(to_state(env, st), a_env, env.tau, env.tau)
    assert ref_obs.is_contiguous()
    # transposition through a workspace, then the fused LDS time-tile kernel: same bits, contiguous row-major results
    for fused, ws in ((False, True), (True, False)):
        env.env_major_fused, env.env_major_workspace = fused, ws
        ws_obs, ws_states, ws_last = env.vmap_sim_ahead(to_state(env, st), a_env, env.tau, env.tau)
        assert ws_obs.is_contiguous() and torch.equal(ws_obs, ref_obs), (fused, ws)
        for n in env.STATE_FIELDS:
            assert torch.equal(getattr(ws_states.physical_state, n), getattr(ref_states.physical_state, n))
            assert torch.equal(getattr(ws_last.physical_state, n), getattr(ref_last.physical_state, n))
    env.env_major_fused, env.env_major_workspace = True, True
    env.traj_layout = "lane_major"
    env.launch_opts = _native.launch_opts(envs_per_lane=vec)  # per-call option (excenv_launch_opts_t), no global state
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), a_lane, env.tau, env.tau)
    assert torch.equal(obs, ref_obs)
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(states.physical_state, n), getattr(ref_states.physical_state, n))
        assert torch.equal(getattr(last.physical_state, n), getattr(ref_last.physical_state, n))


@pytest.mark.parametrize("env_name", ["pendulum", "pmsm", "cartpole"])
def test_per_env_property_arrays(env_name):
    """Static params / normalisation bounds given as [batch_size] arrays (reference test_custom_initialization,
    e.g. tests/envs/pendulum/test_pendulum.py:72-129)."""
    B, K = 777, 20
    dtype = torch.float64
    spec = spec_of(env_name)
    rng = np.random.default_rng(41)
    if env_name == "pendulum":
        spec["params"]["l"] = rng.uniform(0.5, 2.5, B)
        spec["phys_norm"]["omega"] = (rng.uniform(-12, -8, B), 10)
        spec["act_norm"]["torque"] = (-20, rng.uniform(15, 25, B))
    elif env_name == "pmsm":
        spec["params"]["r_s"] = rng.uniform(10e-3, 20e-3, B)
        spec["params"]["p"] = np.full(B, 3.0)
        spec["phys_norm"]["i_q"] = (-250, rng.uniform(200, 300, B))
    else:
        spec["params"]["m_p"] = rng.uniform(0.05, 0.2, B)
        spec["params"]["mu_c"] = rng.uniform(0.0, 0.001, B)
    env, props, keep, _ = make_env(env_name, B, dtype, spec=spec)
    env.sim_ahead_semantics = "step"
    st = random_state(env_name, B, np.float64, spec, seed=42)
    acts = rng.uniform(-1, 1, (B, K, env.action_dim))
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
    o_ref, _, _ = oracle.sim_ahead(env_name, "euler", st, acts, props, spec["tau"])
    assert _close(env_name, obs.cpu().numpy(), o_ref, dtype), max_err(obs.cpu().numpy(), o_ref)
    o1, _ = env.vmap_step(to_state(env, st), torch.as_tensor(acts[:, 0], device=env.device))
    r1, _ = oracle.step(env_name, "euler", st, acts[:, 0], props, spec["tau"])
    assert _close(env_name, o1.cpu().numpy(), r1, dtype)


def test_control_state_reference_columns():
    """generate_observation appends the normalised reference of every control_state name (pendulum_env.py:322-328)."""
    B, K = 512, 9
    env, props, keep, spec = make_env("cartpole", B, torch.float32, control_state=["theta", "deflection"])
    st = random_state("cartpole", B, np.float32, spec, seed=51)
    rng = np.random.default_rng(52)
    refs = {"theta": rng.uniform(-3, 3, B).astype(np.float32), "deflection": rng.uniform(-2, 2, B).astype(np.float32)}
    acts = rng.uniform(-1, 1, (B, K, 1)).astype(np.float32)
    state = to_state(env, st, reference=refs)
    control = [("theta", refs["theta"]), ("deflection", refs["deflection"])]
    assert len(env.obs_description) == 6
    obs, _ = env.vmap_step(state, torch.as_tensor(acts[:, 0], device=env.device))
    o_ref, _ = oracle.step("cartpole", "euler", st, acts[:, 0], props, spec["tau"], control=control)
    assert obs.shape == (B, 6) and _close("cartpole", obs.cpu().numpy(), o_ref, torch.float32)
    for layout in ("lane_major", "env_major"):
        env.traj_layout = layout
        obs, states, last = env.vmap_sim_ahead(state, torch.as_tensor(acts, device=env.device), env.tau, env.tau)
        o_ref, _, _ = oracle.sim_ahead("cartpole", "euler", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD,
                                       control=control)
        assert obs.shape == (B, K + 1, 6) and _close("cartpole", obs.cpu().numpy(), o_ref, torch.float32)
        assert torch.equal(states.reference.theta[:, 3], state.reference.theta)


@pytest.mark.parametrize("env_name", ["pendulum", "fluid_tank", "acrobot"])
def test_substeps_obs_stepsize_smaller_than_action_stepsize(env_name):
    """obs_stepsize < action_stepsize: each action is held for `substeps` solver steps, N+1 = K*substeps+1 rows."""
    B, K, sub = 256, 7, 4
    env, props, keep, spec = make_env(env_name, B, torch.float64, "rk4")
    st = random_state(env_name, B, np.float64, spec, seed=61)
    acts = np.random.default_rng(62).uniform(-1, 1, (B, K, 1))
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device),
                                           env.tau / sub, env.tau)
    o_ref, _, _ = oracle.sim_ahead(env_name, "rk4", st, acts, props, spec["tau"] / sub, env_tau=spec["tau"],
                                   substeps=sub, semantics=oracle.SEM_AHEAD)
    assert obs.shape == (B, K * sub + 1, env.physical_state_dim)
    assert _close(env_name, obs.cpu().numpy(), o_ref, torch.float64), max_err(obs.cpu().numpy(), o_ref)


def test_fluid_tank_empties_step_vs_ahead_semantics():
    """fluid_tank_env.py:146 vs :196 — `step` clips h >= 0 after every step, sim_ahead only clips the saved rows."""
    B, K = 64, 400
    spec = spec_of("fluid_tank")
    spec["tau"] = 5e-2
    spec["act_norm"]["inflow"] = (-0.2, 0.2)  # allows draining below zero
    for sem, osem in (("step", oracle.SEM_STEP), ("ahead", oracle.SEM_AHEAD)):
        env, props, keep, _ = make_env("fluid_tank", B, torch.float32, spec=spec)
        env.sim_ahead_semantics = sem
        st = [np.linspace(0.001, 0.05, B).astype(np.float32)]
        acts = np.random.default_rng(71).uniform(-1, 0.2, (B, K, 1)).astype(np.float32)
        obs, states, last = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
        o_ref, s_ref, _ = oracle.sim_ahead("fluid_tank", "euler", st, acts, props, spec["tau"], semantics=osem)
        assert np.array_equal(obs.cpu().numpy(), o_ref)
        assert float(states.physical_state.height.min()) == 0.0  # the tank did empty


def test_pmsm_deadtime_zero_and_nan_propagation():
    B, K = 256, 12
    spec = spec_of("pmsm")
    spec["params"]["deadtime"] = 0
    for sem, osem in (("step", oracle.SEM_STEP), ("ahead", oracle.SEM_AHEAD)):
        env, props, keep, _ = make_env("pmsm", B, torch.float32, spec=spec)
        env.sim_ahead_semantics = sem
        st = random_state("pmsm", B, np.float32, spec, seed=81)
        acts = np.random.default_rng(82).uniform(-1, 1, (B, K, 2)).astype(np.float32)
        acts[3, 5, 0] = np.nan  # runtime numeric problems surface as NaN, never as exceptions
        obs, _, _ = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
        o_ref, _, _ = oracle.sim_ahead("pmsm", "euler", st, acts, props, spec["tau"], semantics=osem)
        got = obs.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(o_ref))
        assert np.allclose(got, o_ref, rtol=1e-5, atol=1e-5, equal_nan=True)


@pytest.mark.parametrize("deadtime", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pmsm_deadtime_above_one_on_the_step_path(deadtime, dtype):
    """PMSM.step (pmsm_env.py:851-883) treats every deadtime > 0 as a one-step delay (the state holds ONE buffered action) while
    the clip's angle advance uses (deadtime + 0.5) * tau (pmsm_env.py:599-604): vmap_step and the K-exact-steps trajectory
    (EXCENV_SEM_STEP) accept any non-negative integer and agree with the oracle."""
    B, K = 512, 24
    spec = spec_of("pmsm")
    spec["params"]["deadtime"] = deadtime
    env, props, keep, _ = make_env("pmsm", B, dtype, spec=spec)
    env.sim_ahead_semantics = "step"
    st = random_state("pmsm", B, NP_DTYPE[dtype], spec, seed=91)
    acts = np.random.default_rng(92).uniform(-1, 1, (B, K, 2)).astype(NP_DTYPE[dtype])
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    obs1, new = env.vmap_step(to_state(env, st), torch.as_tensor(acts[:, 0], device=env.device))
    o_ref, s_ref = oracle.step("pmsm", "euler", st, acts[:, 0], props, spec["tau"])
    assert np.allclose(obs1.cpu().numpy(), o_ref, rtol=tol, atol=tol)
    assert np.allclose(new.physical_state.u_d_buffer.cpu().numpy(), s_ref[0], rtol=tol, atol=tol * 300)
    # the angle advance really is (deadtime + 0.5) tau: a run with deadtime = 1 clips differently
    spec1 = spec_of("pmsm")
    env1, *_ = make_env("pmsm", B, dtype, spec=spec1)
    _, new1 = env1.vmap_step(to_state(env1, st), torch.as_tensor(acts[:, 0], device=env.device))
    assert not torch.equal(new1.physical_state.u_d_buffer, new.physical_state.u_d_buffer)
    obs, _, last = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
    o_ref, _, l_ref = oracle.sim_ahead("pmsm", "euler", st, acts, props, spec["tau"], semantics=oracle.SEM_STEP)
    assert np.allclose(obs.cpu().numpy(), o_ref, rtol=tol * 10, atol=tol * 10)
    state = to_state(env, st)
    for k in range(K):  # and equals K vmap_step launches bit for bit
        _, state = env.vmap_step(state, torch.as_tensor(acts[:, k], device=env.device))
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(state.physical_state, n), getattr(last.physical_state, n))


def test_single_env_api_and_empty_trajectory():
    """step / sim_ahead for one environment (core_env.py:393-488) and K = 0."""
    env, props1, keep, spec = make_env("pendulum", 1, torch.float64)
    obs, state = env.reset(env.env_properties)
    assert obs.shape == (2,)
    o, s = env.step(state, torch.ones(1), env.env_properties)
    r, _ = oracle.step("pendulum", "euler", [np.array([np.pi]), np.array([0.0])], np.ones((1, 1)), props1, spec["tau"])
    assert np.allclose(o.cpu().numpy(), r[0], rtol=1e-12, atol=1e-12)
    acts = torch.ones((10, 1), dtype=torch.float64)
    obs_t, states, last = env.sim_ahead(state, acts, env.env_properties, env.tau, env.tau)
    assert obs_t.shape == (11, 2) and states.physical_state.theta.shape == (11,)
    from exciting_environments_amd.tree import tree_structure
    assert tree_structure(last) == tree_structure(state)
    env4, _, _, _ = make_env("pendulum", 4, torch.float32)
    _, st4 = env4.vmap_reset()
    o0, s0, l0 = env4.vmap_sim_ahead(st4, torch.empty((4, 0, 1)), env4.tau, env4.tau)
    assert o0.shape == (4, 1, 2)
    assert torch.equal(l0.physical_state.omega, st4.physical_state.omega)


@pytest.mark.parametrize("env_name", ["pmsm", "acrobot", "fluid_tank"])
def test_step_kernel_envs_per_lane_variants_are_bit_identical(env_name):
    from exciting_environments_amd import _native

    B = 4096
    env, props, keep, spec = make_env(env_name, B, torch.float32, "rk4")
    st = random_state(env_name, B, np.float32, spec, seed=91)
    act = torch.as_tensor(np.random.default_rng(92).uniform(-1, 1, (B, env.action_dim)).astype(np.float32), device=env.device)
    outs = []
    for vec in (1, 2, 4):
        env.launch_opts = _native.launch_opts(envs_per_lane=vec)
        outs.append(env.vmap_step(to_state(env, st), act))
        assert _native.last_launch() == f"step_kernel (V={vec})", _native.last_launch()
    for obs, new in outs[1:]:
        assert torch.equal(obs, outs[0][0])
        for n in env.STATE_FIELDS:
            assert torch.equal(getattr(new.physical_state, n), getattr(outs[0][1].physical_state, n))


def test_tiled_layout_is_lane_major_per_tile():
    """EXCENV_LAYOUT_TILED (opt-in): same bits as the lane-major run, tile by tile."""
    B, K = 4096, 21
    env, props, keep, spec = make_env("pmsm", B, torch.float32)
    st = random_state("pmsm", B, np.float32, spec, seed=95)
    acts = torch.as_tensor(np.random.default_rng(96).uniform(-1, 1, (B, K, 2)).astype(np.float32), device=env.device)
    a_lane = env.new_actions_buffer(K)
    a_lane.copy_(acts)
    ref_obs, ref_states, ref_last = env.vmap_sim_ahead(to_state(env, st), a_lane, env.tau, env.tau)
    a_tiled = env.new_actions_buffer(K, layout="tiled")
    a_tiled.copy_(acts.view(B // 1024, 1024, K, 2))
    env.traj_layout = "tiled"
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), a_tiled, env.tau, env.tau)
    assert obs.shape == (B // 1024, 1024, K + 1, 8)
    assert torch.equal(obs.reshape(B, K + 1, 8), ref_obs)
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(states.physical_state, n).reshape(B, K + 1), getattr(ref_states.physical_state, n))
        assert torch.equal(getattr(last.physical_state, n), getattr(ref_last.physical_state, n))


@pytest.mark.parametrize("shape", [(1, 1), (64, 64), (65, 63), (1000, 3), (3, 1000), (4097, 257), (808, 4096), (101, 4096),
                                   (4096, 200), (600, 1028), (1028, 600), (12, 8)])
def test_transpose_kernel(shape):
    from exciting_environments_amd import _native

    for dt in (torch.float32, torch.float64):
        x = torch.randn(shape, dtype=dt, device="cuda")
        assert torch.equal(_native.transpose(x), x.t().contiguous())


def test_error_paths_return_codes_not_faults():
    """Unsupported combinations are rejected by the library with a message (never a fault, never a silent fallback)."""
    import ctypes
    from exciting_environments_amd import _native

    spec = spec_of("pmsm")
    spec["params"]["deadtime"] = 1.5
    env, *_ = make_env("pmsm", 64, torch.float32, spec=spec)
    _, st = env.vmap_reset()
    with pytest.raises(RuntimeError, match="deadtime must be a non-negative integer"):
        env.vmap_step(st, torch.zeros(64, 2, device=env.device))
    spec["params"]["deadtime"] = 2  # the reference's sim_ahead cannot assemble its buffer columns for more than one step
    env, *_ = make_env("pmsm", 64, torch.float32, spec=spec)
    with pytest.raises(RuntimeError, match="EXCENV_SEM_AHEAD supports deadtime 0 or 1"):
        env.vmap_sim_ahead(st, torch.zeros(64, 4, 2, device=env.device), env.tau, env.tau)
    spec = spec_of("pmsm")
    spec["params"]["deadtime"] = np.ones(64)
    env, *_ = make_env("pmsm", 64, torch.float32, spec=spec)
    _, st = env.vmap_reset()
    with pytest.raises(RuntimeError, match="deadtime must be a scalar"):
        env.vmap_step(st, torch.zeros(64, 2, device=env.device))
    env, *_ = make_env("pmsm", 64, torch.float32)
    _, st = env.vmap_reset()
    with pytest.raises(RuntimeError, match="obs_stepsize must equal action_stepsize"):
        env.vmap_sim_ahead(st, torch.zeros(64, 4, 2, device=env.device), env.tau / 2, env.tau)
    with pytest.raises(ValueError, match="integer multiple"):
        env.vmap_sim_ahead(st, torch.zeros(64, 4, 2, device=env.device), env.tau / 1.5, env.tau)
    # misaligned row-major buffers on the step path
    env, *_ = make_env("pendulum", 64, torch.float32)
    _, st = env.vmap_reset()
    props, keep = env._props_for(env.env_properties, 64)
    st_in = [env._t(getattr(st.physical_state, n), (64,)) for n in env.STATE_FIELDS]
    st_out = [torch.empty(64, device=env.device) for _ in st_in]
    act = torch.zeros(65, device=env.device)[1:].view(64, 1)  # 4-byte aligned only
    obs = torch.empty(64, 2, device=env.device)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _native.step(env.ENV_ID, 0, torch.float32, 64, props, None, env.tau, st_in, act, st_out, obs)
    # env-major trajectory longer than the 32-bit per-lane offset allows (generic-stride path, no workspace)
    env.traj_layout, env.env_major_workspace = "env_major", False
    rc = _native.lib().excenv_sim_ahead(
        ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(64), ctypes.c_int64(1 << 21), ctypes.c_int32(1),
        ctypes.byref(props), None, ctypes.c_double(1e-4), ctypes.c_double(1e-4), _native._ptrs(st_in),
        ctypes.c_void_p(obs.data_ptr()), ctypes.c_int(0), ctypes.c_void_p(obs.data_ptr()), None, ctypes.c_int(0),
        _native._ptrs(st_out), ctypes.c_int(0), None, None, None)
    assert rc == -4 and b"too long" in _native.lib().excenv_last_error()
    # the tiled layout needs batch_size % 1024 == 0
    env, *_ = make_env("pendulum", 1000, torch.float32)
    env.traj_layout = "tiled"
    _, st = env.vmap_reset()
    with pytest.raises(AssertionError, match="1024"):
        env.vmap_sim_ahead(st, torch.zeros(1000, 3, 1, device=env.device), env.tau, env.tau)


def test_key_stream_reset_on_device_equals_cpu():
    from exciting_environments_amd import EnvironmentRegistry
    from exciting_environments_amd import random as jr

    keys = jr.split(jr.PRNGKey(5), 64)
    for reg in (EnvironmentRegistry.CART_POLE, EnvironmentRegistry.PMSM):
        o_c, s_c = reg.make(batch_size=64, device="cpu").vmap_reset(keys)
        env = reg.make(batch_size=64, device="cuda")
        o_g, s_g = env.vmap_reset(keys.cuda())
        assert torch.allclose(o_g.cpu(), o_c, atol=1e-6) and torch.equal(s_g.PRNGKey.cpu(), s_c.PRNGKey)
        obs, s1 = env.vmap_step(s_g, torch.zeros(64, env.action_dim, device="cuda"))
        o2, st, last = env.vmap_sim_ahead(s_g, torch.zeros(64, 3, env.action_dim, device="cuda"), env.tau, env.tau)
        assert st.PRNGKey.shape == (64, 4, 2) and torch.equal(last.PRNGKey, s_g.PRNGKey)


def test_observations_only_variant():
    """store_state_trajectory = False: same observations and last_state, no state trajectories written."""
    B, K = 2048, 17
    for layout in ("lane_major", "env_major"):
        env, props, keep, spec = make_env("pmsm", B, torch.float32)
        env.traj_layout = layout
        st = random_state("pmsm", B, np.float32, spec, seed=311)
        acts = torch.as_tensor(np.random.default_rng(312).uniform(-1, 1, (B, K, 2)).astype(np.float32), device=env.device)
        o_full, s_full, l_full = env.vmap_sim_ahead(to_state(env, st), acts, env.tau, env.tau)
        env.store_state_trajectory = False
        o_only, s_only, l_only = env.vmap_sim_ahead(to_state(env, st), acts, env.tau, env.tau)
        assert s_only is None and torch.equal(o_only, o_full)
        for n in env.STATE_FIELDS:
            assert torch.equal(getattr(l_only.physical_state, n), getattr(l_full.physical_state, n))


def test_entry_points_are_hip_graph_capturable():
    """The C ABI only enqueues kernels on the caller's stream (no allocation, no synchronisation): a chain of
    vmap_step / vmap_gym_step / vmap_sim_ahead calls can be captured into a HIP graph and replayed."""
    B, K = 2048, 12
    env, props, keep, spec = make_env("pmsm", B, torch.float32)
    st = random_state("pmsm", B, np.float32, spec, seed=301)
    acts = env.new_actions_buffer(K)
    acts.copy_(torch.as_tensor(np.random.default_rng(302).uniform(-1, 1, (B, K, 2)).astype(np.float32), device=env.device))
    s0 = to_state(env, st)
    # eager reference
    s = s0
    for k in range(4):
        o_ref, s = env.vmap_step(s, acts[:, k].contiguous())
    obs_ref, _, last_ref = env.vmap_sim_ahead(s, acts, env.tau, env.tau)
    a4 = [acts[:, k].contiguous() for k in range(4)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = s0
        for k in range(4):
            o_g, s = env.vmap_step(s, a4[k])
        obs_g, _, last_g = env.vmap_sim_ahead(s, acts, env.tau, env.tau)
    o_g.zero_(); obs_g.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o_g, o_ref) and torch.equal(obs_g, obs_ref)
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(last_g.physical_state, n), getattr(last_ref.physical_state, n))


# ------------------------------------------------------------------------------------------------ device math
def test_device_sincos_fp32_within_2ulp():
    """The in-kernel fp32 sin / cos (devmath.hpp sincos_t). Wrapped angles and a few turns (what the step path sees):
    <= 2 ulp, or <= 4e-9 absolute next to a zero. The whole fast-path range |x| <= 65536 (raw sim_ahead angles grow with
    the trajectory): <= 1e-7 absolute, zeros of sin / cos included; beyond it the device library is exact again."""
    from exciting_environments_amd import _native

    x = torch.cat([torch.linspace(-3.1415927, 3.1415927, 2_000_001), torch.linspace(-50, 50, 500_001),
                   torch.tensor([0.0, -0.0, 1e-30, -1e-20, 3.1415927, -3.1415927, 1.5707964, 1e6, 1e10])]
                  ).to(torch.float32).cuda()
    k = (torch.arange(-40000, 40001, dtype=torch.float64) * (np.pi / 2)).to(torch.float32)
    wide = torch.cat([torch.linspace(-65536.0, 65536.0, 2_000_001), torch.linspace(-70000.0, 70000.0, 200_001), k,
                      torch.nextafter(k, torch.tensor(1e9)), torch.nextafter(k, torch.tensor(-1e9)),
                      torch.tensor([1000.0, 65536.0, 65537.0, -65536.0])]).to(torch.float32).cuda()
    for which, fn in ((0, np.sin), (1, np.cos)):
        got = _native.probe_math(which, x).cpu().numpy().astype(np.float64)
        want = fn(x.cpu().numpy().astype(np.float64))
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got - want) / np.maximum(ulp, 2.0**-149)
        # near the zeros of sin/cos the reduction's absolute error (~1e-9) dominates the shrinking ulp
        ok = (err <= 2.0) | (np.abs(got - want) <= 4e-9)
        assert ok.all(), (which, float(err[~ok].max()))
        got = _native.probe_math(which, wide).cpu().numpy().astype(np.float64)
        want = fn(wide.cpu().numpy().astype(np.float64))
        assert float(np.abs(got - want).max()) <= 1.0e-7, (which, float(np.abs(got - want).max()))


def test_device_wrap_angle_is_python_modulo_bit_exact():
    from exciting_environments_amd import _native

    rng = np.random.default_rng(5)
    for dt, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        pi, two_pi = npdt(np.pi), npdt(2 * np.pi)
        x = np.concatenate([rng.uniform(-10, 10, 1_000_000), rng.uniform(-1e4, 1e4, 200_000),
                            rng.uniform(-1e9, 1e9, 1000), np.arange(-8, 9) * np.pi, np.arange(-8, 9) * 2 * np.pi,
                            [0.0, -0.0, np.pi, -np.pi, 3 * np.pi, 1e-40, -1e-40]]).astype(npdt)
        want = np.remainder(x + pi, two_pi) - pi
        got = _native.probe_math(2, torch.as_tensor(x).cuda()).cpu().numpy()
        assert got.dtype == want.dtype
        assert np.array_equal(got, want), (dt, int((got != want).sum()))
        for bad in (np.nan, np.inf, -np.inf):
            assert np.isnan(_native.probe_math(2, torch.tensor([bad], dtype=dt).cuda()).item())


HALF_PI_LD = np.longdouble("1.57079632679489661923132169163975144")
# |x| up to which devmath.hpp documents sincos_lean, with the bound of each range (the header's figures)
LEAN_RANGES = ((1.6e6, 2e-16), (1e10, 2e-16), (1e12, 4e-15))


def _trig_error(fn, x, got, subsample=4000):
    """|got - sin / cos(x)| for float64 points against extended precision: np.longdouble where it carries more than 60 bits (x87),
    else mpmath on a subsample, the subtraction inside mpmath so that the reference is never rounded to a double (which alone would
    cost half an ulp, 1.1e-16, of bounds of 2e-16) -> (error, reference rounded to float64, indices of the points covered)"""
    if np.finfo(np.longdouble).eps < 1e-18:
        with np.errstate(invalid="ignore"):
            want = {"sin": np.sin, "cos": np.cos}[fn](x.astype(np.longdouble))
        return np.abs(got.astype(np.longdouble) - want).astype(np.float64), want.astype(np.float64), np.arange(x.size)
    import mpmath

    mpmath.mp.prec = 120
    idx = np.unique(np.concatenate([np.linspace(0, x.size - 1, subsample).astype(np.int64), np.arange(min(x.size, 64))]))
    f = {"sin": mpmath.sin, "cos": mpmath.cos}[fn]
    err, want = np.full(idx.size, np.nan), np.full(idx.size, np.nan)
    for i, (v, g) in enumerate(zip(x[idx], got[idx])):
        if np.isfinite(v) and np.isfinite(g):
            ref = f(mpmath.mpf(float(v)))
            err[i], want[i] = float(abs(mpmath.mpf(float(g)) - ref)), float(ref)
    return err, want, idx


def _lean_points(limit, n=200_000, seed=11):
    """Both signs: log-spaced magnitudes up to `limit`, and multiples of pi/2 up to it with both neighbours"""
    rng = np.random.default_rng(seed)
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(limit), n))
    k = np.round(np.exp(rng.uniform(0.0, np.log(limit / (np.pi / 2)), n // 4))).astype(np.longdouble)
    near = (k * HALF_PI_LD).astype(np.float64)
    near = near[near <= limit]
    x = np.concatenate([mag, near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf), [limit]])
    return np.concatenate([x, -x])


def test_device_sincos_lean_fp64_within_its_documented_error():
    """devmath.hpp sincos_lean, the fp64 sin / cos of the four differentiable kernels (probe 3 / 4), against extended precision:
    absolute error <= 2e-16 on wrapped angles, a few turns, the neighbours of k pi/2 for |k| <= 40 000 and every magnitude up to
    1.6e6 (the source's first claim; tools/sincos_lean_restate.c measures 1.2e-16 on the CPU), and the header's bounds beyond:
    <= 2e-16 up to 1e10, <= 4e-15 up to 1e12. The angle of a caller is not wrapped ("ahead" rows, row 0 under "step"): with the
    quadrant taken from (int)n the last two ranges gave errors of 2.0 from |x| = 2^31 pi/2 = 3.37e9 on. NaN and inf give NaN;
    the routine exists in fp64 only."""
    from exciting_environments_amd import _native

    k = (np.arange(-40000, 40001).astype(np.longdouble) * HALF_PI_LD).astype(np.float64)
    dense = np.concatenate([np.linspace(-np.pi, np.pi, 2_000_001), np.linspace(-50.0, 50.0, 500_001), k, np.nextafter(k, np.inf),
                            np.nextafter(k, -np.inf), [0.0, -0.0, 1e-300, -1e-200]])
    sets = [("wrapped, +-50 and k pi/2", dense, 2e-16)]
    sets += [(f"|x| <= {limit:g}", _lean_points(limit), bound) for limit, bound in LEAN_RANGES]
    for name, x, bound in sets:
        xd = torch.as_tensor(x, dtype=torch.float64).cuda()
        for which, fn in ((3, "sin"), (4, "cos")):
            got = _native.probe_math(which, xd).cpu().numpy()
            err = float(_trig_error(fn, x, got)[0].max())
            print(f"sincos_lean {fn} {name}: {x.size} points, worst absolute error {err:.3e}, bound {bound:.1e}")
            assert np.isfinite(got).all() and err <= bound, (name, fn, err)
    bad = torch.tensor([np.nan, np.inf, -np.inf], dtype=torch.float64).cuda()
    for which in (3, 4):
        assert bool(torch.isnan(_native.probe_math(which, bad)).all())
        zero = _native.probe_math(which, torch.tensor([0.0, -0.0], dtype=torch.float64).cuda()).cpu().numpy()
        assert np.array_equal(zero, [0.0, 0.0] if which == 3 else [1.0, 1.0])
        with pytest.raises(RuntimeError):
            _native.probe_math(which, torch.zeros(4, dtype=torch.float32).cuda())


def test_device_sincos_fp64_within_2ulp():
    """The forward kernels' fp64 sin / cos (devmath.hpp sin_t / cos_t in fp64: the device library) on wrapped angles and a few
    turns: <= 2 ulp, or <= 4e-25 absolute next to a zero."""
    from exciting_environments_amd import _native

    k = (np.arange(-32, 33).astype(np.longdouble) * HALF_PI_LD).astype(np.float64)
    x = np.concatenate([np.linspace(-np.pi, np.pi, 2_000_001), np.linspace(-50.0, 50.0, 500_001), k, np.nextafter(k, np.inf),
                        np.nextafter(k, -np.inf), [0.0, -0.0, 1e-300, -1e-200, np.pi, -np.pi, np.pi / 2]])
    xd = torch.as_tensor(x, dtype=torch.float64).cuda()
    for which, fn in ((0, "sin"), (1, "cos")):
        got = _native.probe_math(which, xd).cpu().numpy()
        diff, want, idx = _trig_error(fn, x, got)
        ulp = np.maximum(np.spacing(np.abs(want)), 2.0 ** -1074)
        ok = (diff <= 2.0 * ulp) | (diff <= 4e-25)
        print(f"fp64 {fn}: {x.size} points, worst {float((diff / ulp).max()):.3f} ulp")
        assert ok.all(), (fn, float((diff / ulp)[~ok].max()))


@pytest.mark.parametrize("dt,npdt", [(torch.float32, np.float32), (torch.float64, np.float64)], ids=["float32", "float64"])
def test_device_wrap_angle_at_the_turn_boundaries_and_in_mixed_waves(dt, npdt):
    """pymod_two_pi estimates the truncated quotient with a reciprocal multiply, off by at most one: the places where it is off are
    the neighbours of 2 pi k. theta = 2 pi k and 2 pi k - pi (so that theta + pi is next to a multiple) with their +-1 and +-2 ulp
    neighbours, k over the powers of two and random k up to 2^22, both signs; then a mixed wave: one value past the guard
    (|theta| >= 2.64e7: the library's remainder loop) per 64 at lane 0, 31 or 63 among ordinary angles. np.remainder is the
    reference, bit for bit."""
    from exciting_environments_amd import _native
    from helpers_cold import MOD_LIMIT

    rng = np.random.default_rng(6)
    pi, two_pi = npdt(np.pi), npdt(2 * np.pi)
    k = np.concatenate([2.0 ** np.arange(0, 23), rng.integers(1, 1 << 22, 200_000).astype(np.float64)]).astype(npdt)
    base = np.concatenate([k * two_pi, k * two_pi - pi])
    base = np.concatenate([base, -base])
    pts = [base]
    for direction in (np.inf, -np.inf):
        one = np.nextafter(base, npdt(direction))
        pts += [one, np.nextafter(one, npdt(direction))]
    x = np.concatenate(pts).astype(npdt)
    want = np.remainder(x + pi, two_pi) - pi
    got = _native.probe_math(2, torch.as_tensor(x).cuda()).cpu().numpy()
    assert got.dtype == want.dtype
    print(f"wrap_angle {npdt.__name__}: {x.size} points next to 2 pi k, {int((got != want).sum())} differ")
    assert np.array_equal(got, want), int((got != want).sum())
    # mixed waves
    x = rng.uniform(-10, 10, 64 * 300).astype(npdt)
    for w in range(300):
        x[64 * w + (0, 31, 63)[w % 3]] = npdt((-1) ** w * rng.uniform(1.01 * MOD_LIMIT, 1e9))
    assert (np.abs(x) >= MOD_LIMIT).sum() == 300
    want = np.remainder(x + pi, two_pi) - pi
    got = _native.probe_math(2, torch.as_tensor(x).cuda()).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_invariant_division_in_a_mixed_wave(dtype):
    """InvDiv::div's guard is a wave-wide ballot and the plain division is then selected per lane: one quotient per 64 outside
    the window (a zero numerator, 2^70 / 2^-70 in fp32 or 2^500 / 2^-500 in fp64, NaN) at lane 0, 31 or 63, the rest inside.
    Every lane has the bits of the plain division."""
    from exciting_environments_amd import _native

    g = torch.Generator(device="cuda")
    g.manual_seed(78)
    n = 64 * 3000
    it = torch.int32 if dtype == torch.float32 else torch.int64
    big = 70 if dtype == torch.float32 else 500
    num = torch.ldexp(torch.rand(n, generator=g, dtype=dtype, device="cuda") + 1.0, torch.randint(-20, 21, (n,), generator=g, device="cuda"))
    den = torch.ldexp(torch.rand(n, generator=g, dtype=dtype, device="cuda") + 1.0, torch.randint(-20, 21, (n,), generator=g, device="cuda"))
    num = num * (torch.randint(0, 2, (n,), generator=g, device="cuda").to(dtype) * 2 - 1)
    w = torch.arange(n // 64, device="cuda")
    at = 64 * w + torch.tensor([0, 31, 63], device="cuda")[w % 3]
    kind = (w // 3) % 3
    num[at] = torch.where(kind == 0, torch.zeros((), dtype=dtype, device="cuda"),
                          torch.where(kind == 1, torch.full((), 2.0 ** big, dtype=dtype, device="cuda"),
                                      torch.full((), float("nan"), dtype=dtype, device="cuda")))
    den[at] = torch.where(kind == 1, torch.full((), 2.0 ** -big, dtype=dtype, device="cuda"), den[at])
    fast, ref = _native.probe_div(num, den)
    same = (fast.view(it) == ref.view(it)) | (torch.isnan(fast) & torch.isnan(ref))
    assert bool(same.all()), (num[~same][:4], den[~same][:4], fast[~same][:4], ref[~same][:4])
    assert bool(torch.isnan(ref[at][kind == 2]).all()) and bool((ref[at][kind == 0] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_invariant_division_has_the_bits_of_plain_division(dtype):
    """devmath.hpp InvDiv (division by a loop-invariant denominator: precomputed refined reciprocal + the compiler's own
    residual FMAs) against `a / b` as hipcc expands it, bit for bit: random operands over the whole exponent range, operands
    in the moderate range the fast path serves, exact quotients, and the special values (0, -0, inf, nan, denormals)."""
    from exciting_environments_amd import _native

    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    n = 1 << 22
    fi = torch.finfo(dtype)
    it = torch.int32 if dtype == torch.float32 else torch.int64

    def rand_float(lo_exp, hi_exp):
        m = torch.rand(n, generator=g, dtype=dtype, device="cuda") + 1.0
        e = torch.randint(lo_exp, hi_exp + 1, (n,), generator=g, device="cuda")
        s = torch.randint(0, 2, (n,), generator=g, device="cuda").to(dtype) * 2 - 1
        return torch.ldexp(m * s, e)

    emax = 126 if dtype == torch.float32 else 1021
    cases = [
        (rand_float(-20, 20), rand_float(-20, 20)),                      # the regime of the environments
        (rand_float(-emax, emax), rand_float(-emax, emax)),              # everything, incl. overflow / underflow of the quotient
        (rand_float(-emax, emax), rand_float(-30, 30)),
        (rand_float(-30, 30) * 0 + rand_float(0, 0), rand_float(-10, 10)),
    ]
    a = rand_float(-8, 8)
    b = torch.round(rand_float(0, 6))
    cases.append((a * b, b))                                             # exactly representable quotients
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), fi.tiny, -fi.tiny, fi.tiny / 8, fi.max, -fi.max,
                            1.0, -1.0, 3.0, 1e-30 if dtype == torch.float32 else 1e-300, fi.eps], dtype=dtype, device="cuda")
    sa, sb = torch.meshgrid(special, special, indexing="ij")
    cases.append((sa.reshape(-1), sb.reshape(-1)))
    cases.append((rand_float(-20, 20), special[torch.randint(0, special.numel(), (n,), generator=g, device="cuda")]))
    cases.append((special[torch.randint(0, special.numel(), (n,), generator=g, device="cuda")], rand_float(-20, 20)))
    for num, den in cases:
        fast, ref = _native.probe_div(num, den)
        both_nan = torch.isnan(fast) & torch.isnan(ref)
        same = (fast.view(it) == ref.view(it)) | both_nan
        assert bool(same.all()), (num[~same][:4], den[~same][:4], fast[~same][:4], ref[~same][:4])
    # and the compiler's division is the correctly rounded one (what the CPU oracle computes)
    num, den = cases[0]
    fast, _ = _native.probe_div(num, den)
    assert np.array_equal(fast.cpu().numpy(), num.cpu().numpy() / den.cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B", [4096, 1003])
def test_control_columns_with_the_vectorised_kernels_equal_the_general_kernel(B, dtype):
    """control_state with broadcast properties: the lean sim_ahead_kernel writes the trajectory and control_fill_kernel the
    constant reference columns (launch.hpp split_control). Must equal, bit for bit, what the one-environment-per-lane GENERAL
    kernel writes — forced here by a per-environment property array holding the same value — in the lane-major and the tiled
    layout, for every lane width, for a ragged batch (scalar fill) and in both dtypes."""
    from exciting_environments_amd import EnvironmentRegistry, _native

    K = 11
    kw = dict(batch_size=B, device="cuda:0", dtype=dtype, control_state=["i_d", "torque"])
    env = EnvironmentRegistry.PMSM.make(**kw)
    sp = env.env_properties.static_params
    per_env = {k: getattr(sp, k) for k in sp.__dataclass_fields__}
    per_env["r_s"] = np.full(B, float(sp.r_s))
    env_g = EnvironmentRegistry.PMSM.make(static_params=per_env, **kw)
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    _, st = env.vmap_reset()
    ref = {n: torch.full((B,), float("nan"), dtype=dtype, device="cuda") for n in env.STATE_FIELDS}
    ref["i_d"] = -torch.rand(B, generator=g, device="cuda", dtype=dtype) * 200
    ref["torque"] = (torch.rand(B, generator=g, device="cuda", dtype=dtype) - 0.5) * 300
    from dataclasses import replace
    st = replace(st, reference=env.PhysicalState(**ref))
    acts = env.new_actions_buffer(K)
    acts.copy_(torch.rand((B, K, 2), generator=g, device="cuda", dtype=dtype) * 2 - 1)
    obs_g, st_g, last_g = env_g.vmap_sim_ahead(st, acts, env.tau, env.tau)
    assert obs_g.shape == (B, K + 1, 10)
    want_id = 2 * (ref["i_d"] - (-250.0)) / (0.0 - (-250.0)) - 1
    assert torch.allclose(obs_g[:, 5, 8], want_id, rtol=1e-6, atol=1e-6) and torch.equal(obs_g[:, 0, 9], obs_g[:, K, 9])
    vmax = 4 if dtype == torch.float32 else 2
    for vec in (1, 2, 4):
        if vec > vmax or B % vec:
            continue
        env.launch_opts = _native.launch_opts(envs_per_lane=vec)
        obs, stt, last = env.vmap_sim_ahead(st, acts, env.tau, env.tau)
        assert torch.equal(obs, obs_g), (vec, float((obs - obs_g).abs().max()))
        assert torch.equal(stt.physical_state.i_q, st_g.physical_state.i_q)
        assert torch.equal(last.physical_state.epsilon, last_g.physical_state.epsilon)
    if B % 1024 == 0 and dtype == torch.float32:
        env.launch_opts = None
        env.traj_layout = "tiled"
        obs_t, _, _ = env.vmap_sim_ahead(st, acts, env.tau, env.tau)
        assert torch.equal(obs_t.reshape(B, K + 1, 10), obs_g)


@pytest.mark.parametrize("env_name", ["pendulum", "acrobot", "cartpole"])
@pytest.mark.parametrize("solver", ["euler", "tsit5"])
def test_unwrapped_angles_far_outside_the_principal_range(env_name, solver):
    """sim_ahead (SEM_AHEAD) integrates the RAW angle: it is wrapped only in the saved rows (pendulum_env.py:243-259), so a long
    trajectory — or a caller's unwrapped initial state — feeds sin / cos with |x| of tens of thousands. The fp32 kernels serve
    that range from their fast path (|x| <= 65 536, <= 1e-7 absolute) and the library beyond: both against the fp32 oracle."""
    B, K = 1024, 48
    env, props, keep, spec = make_env(env_name, B, torch.float32, solver)
    st = random_state(env_name, B, np.float32, spec, seed=901)
    rng = np.random.default_rng(902)
    big = np.concatenate([rng.uniform(-6.0e4, 6.0e4, B - 64), rng.uniform(-3.0e5, 3.0e5, 64)]).astype(np.float32)
    angle = {"pendulum": "theta", "acrobot": "theta_1", "cartpole": "theta"}[env_name]
    st[list(oracle.STATE_FIELDS[env_name]).index(angle)] = big
    acts = rng.uniform(-1, 1, (B, K, 1)).astype(np.float32)
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
    o_ref, s_ref, _ = oracle.sim_ahead(env_name, solver, st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD)
    got, want = obs.cpu().numpy(), o_ref
    assert np.isfinite(got).all()
    # the rows are wrapped from angles of magnitude 1e4..3e5 (fp32 spacing up to 0.03 rad): identical wrap on both sides, and
    # the velocities differ only through sin / cos (1e-7 absolute per evaluation, amplified by the dynamics over 48 steps)
    err = np.abs(got - want)
    cols = ANGLE_OBS.get(env_name, [])
    for c in cols:  # normalised angles: compare on the circle
        err[..., c] = np.minimum(err[..., c], 2.0 - err[..., c])
    assert float(err.max()) <= 2e-4, float(err.max())


@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_state_structure_is_stable_through_step_and_sim_ahead_for_tsit5(env_name):
    """The pytree structure of a State — including the (first_step, f0) solver-state pair of an FSAL solver, e.g.
    pendulum_env.py:177-192, 249-251 — is the same after reset, vmap_step and vmap_sim_ahead (last_state and the trajectory)."""
    from exciting_environments_amd.tree import tree_flatten, tree_structure

    B, K = 64, 5
    env, props, keep, spec = make_env(env_name, B, torch.float32, solver="tsit5")
    _, s0 = env.vmap_reset()
    act = torch.zeros((B, env.action_dim), device=env.device)
    _, s1 = env.vmap_step(s0, act)
    _, traj, last = env.vmap_sim_ahead(s1, torch.zeros((B, K, env.action_dim), device=env.device), env.tau, env.tau)
    assert tree_structure(s1) == tree_structure(s0) == tree_structure(last) == tree_structure(traj)
    assert s0.additions.solver_state is not None
    assert all(tuple(l.shape) == (B, K + 1) for l in tree_flatten(traj.additions.solver_state)[0])
    _, s2 = env.vmap_step(last, act)  # a state that came out of a trajectory steps on
    assert tree_structure(s2) == tree_structure(s0)


@pytest.mark.parametrize("env_name,dtype,B,K", [("pmsm", torch.float32, 8192, 26), ("pmsm", torch.float64, 4100, 17),
                                                ("pendulum", torch.float32, 8260, 24), ("cartpole", torch.float64, 6000, 256),
                                                ("pendulum", torch.float32, 8192, 25)])
def test_row_major_actions_of_large_batches_equal_lane_major_actions(env_name, dtype, B, K):
    """Reference-shaped [B, K, A] actions with the default trajectories: the library transposes them through scratch memory —
    batches >= 4096 with short rows made of whole 16-byte pieces take the row-block form of the transposition
    (csrc/transpose.hip), the last case (K * A = 25 words) the general one. Same bits as lane-major actions."""
    env, props, keep, spec = make_env(env_name, B, dtype)
    st = random_state(env_name, B, NP_DTYPE[dtype], spec, seed=71)
    acts = np.random.default_rng(72).uniform(-1, 1, (B, K, env.action_dim)).astype(NP_DTYPE[dtype])
    a_row = torch.as_tensor(acts, device=env.device)
    a_lane = env.new_actions_buffer(K)
    a_lane.copy_(a_row)
    assert a_row.is_contiguous() and not a_lane.is_contiguous()
    o1, s1, l1 = env.vmap_sim_ahead(to_state(env, st), a_row, env.tau, env.tau)
    o2, s2, l2 = env.vmap_sim_ahead(to_state(env, st), a_lane, env.tau, env.tau)
    assert torch.equal(o1, o2)
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(s1.physical_state, n), getattr(s2.physical_state, n))
        assert torch.equal(getattr(l1.physical_state, n), getattr(l2.physical_state, n))
