"""sim_ahead_semantics = "ahead_accumulated_t" (EXCENV_SEM_AHEAD_ACCUMULATED_T) on the GPU against the CPU oracle's restatement of
diffrax's loop (oracle.SEM_AHEAD_ACCUMULATED_T, same integer value): every model, solver and dtype, every kernel form the planner
can pick for it, the layouts, substeps, PMSM dead time, the fused gym outputs, chained chunks and the C ABI's edges. The action row
does not depend on the state, so the tolerances are those of tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from conftest import ENV_NAMES
from helpers import (ANGLE_OBS, ANGLE_STATES, NP_DTYPE, TRIG_FREE, circ_close, make_env, max_err, random_state, spec_of,
                     to_state)

pytestmark = pytest.mark.gpu

ACC = "ahead_accumulated_t"
SOLVERS = ["euler", "rk4", "tsit5"]


def _tol(env, dtype):
    if env in TRIG_FREE:
        return 0.0, 0.0
    return (1e-9, 1e-9) if dtype == torch.float64 else (1e-5, 1e-5)


def _close(env, got, want, dtype):
    rtol, atol = _tol(env, dtype)
    if rtol == 0.0:
        return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)
    return circ_close(got, want, ANGLE_OBS.get(env, []), rtol, atol)


def _states_close(env_name, env, states, s_ref, dtype):
    rtol, atol = _tol(env_name, dtype)
    for j, n in enumerate(env.STATE_FIELDS):
        got = getattr(states.physical_state, n).cpu().numpy()
        scale = max(1.0, float(np.nanmax(np.abs(s_ref[j]))))
        if rtol == 0:
            assert np.array_equal(got, s_ref[j]), n
        elif j in ANGLE_STATES.get(env_name, []):
            assert circ_close(got[..., None], s_ref[j][..., None], [0], rtol, atol * scale, period=2 * np.pi), n
        else:
            assert np.allclose(got, s_ref[j], rtol=rtol, atol=atol * scale), (n, max_err(got, s_ref[j]))


def _last():
    from exciting_environments_amd import _native
    return _native.last_launch()


def _problem(env_name, B, K, dtype, solver="euler", seed=0, spec=None, control_state=None):
    env, props, keep, spec = make_env(env_name, B, dtype, solver, spec=spec, control_state=control_state)
    env.sim_ahead_semantics = ACC
    st = random_state(env_name, B, NP_DTYPE[dtype], spec, seed=seed)
    acts = np.random.default_rng(seed + 1).uniform(-1, 1, (B, K, env.action_dim)).astype(NP_DTYPE[dtype])
    return env, props, keep, spec, st, acts


def _lane_actions(env, acts):
    a = env.new_actions_buffer(acts.shape[1])
    a.copy_(torch.as_tensor(acts, device=env.device))
    return a


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_matches_the_oracle(env_name, solver, dtype):
    """One environment per lane (what the batch rule gives B = 2048); the wider lanes of every instantiation are held against this
    form in tests/test_gpu_lean_forms.py."""
    B, K = 2048, 64
    env, props, keep, spec, st, acts = _problem(env_name, B, K, dtype, solver, seed=301)
    obs, states, last = env.vmap_sim_ahead(to_state(env, st), _lane_actions(env, acts), env.tau, env.tau)
    assert _last() == "sim_ahead_kernel (V=1, accumulated t)", _last()
    o_ref, s_ref, l_ref = oracle.sim_ahead(env_name, solver, st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert oracle.SEM_AHEAD_ACCUMULATED_T == 2
    assert tuple(obs.shape) == o_ref.shape == (B, K + 1, o_ref.shape[-1])
    assert _close(env_name, obs.cpu().numpy(), o_ref, dtype), max_err(obs.cpu().numpy(), o_ref)
    _states_close(env_name, env, states, s_ref, dtype)
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(last.physical_state, n), getattr(states.physical_state, n)[:, -1])


@pytest.mark.parametrize("env_name", ["pmsm", "pendulum", "mass_spring_damper"])
def test_envs_per_lane_are_bit_identical(env_name):
    from exciting_environments_amd import _native

    B, K = 1024, 33
    env, props, keep, spec, st, acts = _problem(env_name, B, K, torch.float32, seed=311)
    a = _lane_actions(env, acts)
    runs = []
    for vec in (1, 2, 4):
        env.launch_opts = _native.launch_opts(envs_per_lane=vec)
        obs, states, last = env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
        assert _last() == f"sim_ahead_kernel (V={vec}, accumulated t)", _last()
        runs.append((obs, states))
    for obs, states in runs[1:]:
        assert torch.equal(obs, runs[0][0])
        for n in env.STATE_FIELDS:
            assert torch.equal(getattr(states.physical_state, n), getattr(runs[0][1].physical_state, n))
    o_ref, _, _ = oracle.sim_ahead(env_name, "euler", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert _close(env_name, runs[0][0].cpu().numpy(), o_ref, torch.float32), max_err(runs[0][0].cpu().numpy(), o_ref)


def test_wide_workgroups():
    """pendulum Euler fp32 at B = 2^20: four environments per lane in 1024-thread workgroups (kernels.hpp NT)."""
    from exciting_environments_amd import _native

    B, K = 1 << 20, 8
    env, props, keep, spec, st, acts = _problem("pendulum", B, K, torch.float32, seed=321)
    a = _lane_actions(env, acts)
    obs, states, _ = env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
    assert _last() == "sim_ahead_kernel (V=4, 1024 threads, accumulated t)", _last()
    obs = obs.cpu().numpy()
    env.launch_opts = _native.launch_opts(envs_per_lane=1)
    obs1, _, _ = env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
    assert _last() == "sim_ahead_kernel (V=1, accumulated t)", _last()
    assert np.array_equal(obs, obs1.cpu().numpy())
    sl = slice(0, 1 << 14)
    o_ref, _, _ = oracle.sim_ahead("pendulum", "euler", [s[sl] for s in st], acts[sl], props_slice(props, "pendulum", spec, sl),
                                   spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert _close("pendulum", obs[sl], o_ref, torch.float32), max_err(obs[sl], o_ref)


def props_slice(props, env_name, spec, sl):
    p, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float32, sl.stop - sl.start)
    props_slice.keep = keep
    return p


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_general_kernel_per_env_properties(dtype):
    B, K = 777, 20
    spec = spec_of("pendulum")
    rng = np.random.default_rng(331)
    spec["params"]["l"] = rng.uniform(0.5, 2.5, B)
    spec["act_norm"]["torque"] = (-20, rng.uniform(15, 25, B))
    env, props, keep, spec, st, acts = _problem("pendulum", B, K, dtype, "rk4", seed=332, spec=spec)
    obs, states, _ = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
    assert _last() in ("sim_ahead_kernel (general, accumulated t)", "transposition workspace + sim_ahead_kernel (accumulated t)"), _last()
    o_ref, s_ref, _ = oracle.sim_ahead("pendulum", "rk4", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert _close("pendulum", obs.cpu().numpy(), o_ref, dtype), max_err(obs.cpu().numpy(), o_ref)
    _states_close("pendulum", env, states, s_ref, dtype)


def test_general_kernel_control_columns():
    B, K = 512, 9
    cs = ["theta", "deflection"]
    env, props, keep, spec, st, acts = _problem("cartpole", B, K, torch.float64, "tsit5", seed=341, control_state=cs)
    rng = np.random.default_rng(342)
    refs = {"theta": rng.uniform(-3, 3, B), "deflection": rng.uniform(-2, 2, B)}
    obs, _, _ = env.vmap_sim_ahead(to_state(env, st, reference=refs), _lane_actions(env, acts), env.tau, env.tau)
    assert _last().endswith("accumulated t)"), _last()
    o_ref, _, _ = oracle.sim_ahead("cartpole", "tsit5", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T,
                                   control=[(n, refs[n]) for n in cs])
    assert obs.shape[-1] == o_ref.shape[-1] == 4 + 2
    assert _close("cartpole", obs.cpu().numpy(), o_ref, torch.float64), max_err(obs.cpu().numpy(), o_ref)


@pytest.mark.parametrize("env_name,dtype", [("mass_spring_damper", torch.float32), ("fluid_tank", torch.float64),
                                            ("pendulum", torch.float64)])
def test_fused_rew_trunc_term(env_name, dtype):
    """return_rew_trunc_term=True: the gym outputs of the launch against the oracle's reward / flags of the oracle's own trajectory."""
    B, K = 700, 24
    env, props, keep, spec, st, acts = _problem(env_name, B, K, dtype, seed=351)
    obs, states, last, reward, truncated, terminated = env.vmap_sim_ahead(
        to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau, return_rew_trunc_term=True)
    assert _last() == "sim_ahead_kernel (general, accumulated t)", _last()
    o_ref, s_ref, _ = oracle.sim_ahead(env_name, "euler", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert _close(env_name, obs.cpu().numpy(), o_ref, dtype)
    r_ref, tr_ref, te_ref = oracle.rew_trunc_term_ahead(env_name, s_ref, props)
    rtol, atol = _tol(env_name, dtype)
    if rtol == 0.0:
        assert np.array_equal(reward.cpu().numpy(), r_ref)
    else:
        assert np.allclose(reward.cpu().numpy(), r_ref, rtol=rtol, atol=atol), max_err(reward.cpu().numpy(), r_ref)
    assert np.array_equal(truncated.cpu().numpy(), tr_ref) and np.array_equal(terminated.cpu().numpy(), te_ref)


@pytest.mark.parametrize("workspace", [True, False])
def test_env_major_trajectories(workspace):
    B, K = 1024, 40
    env, props, keep, spec, st, acts = _problem("pmsm", B, K, torch.float32, seed=361)
    env.traj_layout = "env_major"
    env.env_major_workspace = workspace
    obs, states, _ = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
    assert obs.is_contiguous()
    assert _last() == ("transposition workspace + sim_ahead_kernel (accumulated t)" if workspace
                       else "sim_ahead_kernel (V=1, accumulated t)"), _last()
    o_ref, s_ref, _ = oracle.sim_ahead("pmsm", "euler", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert _close("pmsm", obs.cpu().numpy(), o_ref, torch.float32), max_err(obs.cpu().numpy(), o_ref)
    _states_close("pmsm", env, states, s_ref, torch.float32)


def test_row_major_actions_lane_major_outputs():
    """actions[B, K, A] as the reference passes them: AEM under "ahead", the transposition workspace here."""
    B, K = 1 << 18, 16
    env, props, keep, spec, st, acts = _problem("mass_spring_damper", B, K, torch.float32, seed=371)
    a = torch.as_tensor(acts, device=env.device)
    env.sim_ahead_semantics = "ahead"
    env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
    assert _last() == "sim_ahead_kernel (row-major actions fused)", _last()
    env.sim_ahead_semantics = ACC
    obs, _, _ = env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
    assert _last() == "transposition workspace + sim_ahead_kernel (accumulated t)", _last()
    o_ref, _, _ = oracle.sim_ahead("mass_spring_damper", "euler", st, acts, props, spec["tau"],
                                   semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert np.array_equal(obs.cpu().numpy(), o_ref)


@pytest.mark.parametrize("env_name", ["pendulum", "fluid_tank", "acrobot"])
def test_substeps(env_name):
    B, K, sub = 256, 7, 4
    env, props, keep, spec, st, acts = _problem(env_name, B, K, torch.float64, "rk4", seed=381)
    obs, _, _ = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau / sub, env.tau)
    assert _last().endswith("accumulated t)"), _last()
    o_ref, _, _ = oracle.sim_ahead(env_name, "rk4", st, acts, props, spec["tau"] / sub, env_tau=spec["tau"], substeps=sub,
                                   semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert obs.shape == (B, K * sub + 1, o_ref.shape[-1])
    assert _close(env_name, obs.cpu().numpy(), o_ref, torch.float64), max_err(obs.cpu().numpy(), o_ref)


@pytest.mark.parametrize("deadtime", [0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pmsm_deadtime(deadtime, dtype):
    B, K = 512, 100
    spec = spec_of("pmsm")
    spec["params"]["deadtime"] = deadtime
    env, props, keep, spec, st, acts = _problem("pmsm", B, K, dtype, seed=391, spec=spec)
    if deadtime > 1:
        with pytest.raises(RuntimeError, match="deadtime 0 or 1"):
            env.vmap_sim_ahead(to_state(env, st), _lane_actions(env, acts), env.tau, env.tau)
        return
    obs, states, _ = env.vmap_sim_ahead(to_state(env, st), _lane_actions(env, acts), env.tau, env.tau)
    assert _last().endswith("accumulated t)"), _last()
    o_ref, s_ref, _ = oracle.sim_ahead("pmsm", "euler", st, acts, props, spec["tau"], semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
    assert _close("pmsm", obs.cpu().numpy(), o_ref, dtype), max_err(obs.cpu().numpy(), o_ref)
    _states_close("pmsm", env, states, s_ref, dtype)


def test_it_changes_the_trajectory():
    """PMSM fp32, the C3 chunk shape (100 steps, tau 1e-4): most rows differ from the default semantics."""
    B, K = 2048, 100
    env, props, keep, spec, st, acts = _problem("pmsm", B, K, torch.float32, seed=401)
    assert spec["tau"] == 1e-4
    a = _lane_actions(env, acts)
    acc, _, _ = env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
    env.sim_ahead_semantics = "ahead"
    ahead, _, _ = env.vmap_sim_ahead(to_state(env, st), a, env.tau, env.tau)
    differ = (acc != ahead).any(dim=2).any(dim=0).cpu().numpy()
    assert not differ[0] and differ.sum() >= 80, differ.sum()


def test_raw_abi_values():
    from exciting_environments_amd import _native

    B, K = 256, 5
    env, props, keep, spec, st, acts = _problem("pendulum", B, K, torch.float32, seed=411)
    dev = env.device
    p, pk = oracle.make_props("pendulum", spec["params"], spec["phys_norm"], spec["act_norm"], np.float32, B)
    packed, keep2 = env._props_for(env.env_properties, B)
    st_in = [torch.as_tensor(s, device=dev) for s in st]
    a = torch.as_tensor(acts, device=dev)
    obs = torch.empty((B, K + 1, 2), dtype=torch.float32, device=dev)
    last = [torch.empty(B, dtype=torch.float32, device=dev) for _ in st]
    args = (env.ENV_ID, 0, torch.float32, B, K, 1, packed, None, float(env.tau), float(env.tau), st_in, a,
            _native.LAYOUT_ENV_MAJOR, obs, None, _native.LAYOUT_ENV_MAJOR, last)
    _native.sim_ahead(*args, _native.SEM_AHEAD_ACCUMULATED_T)
    torch.cuda.synchronize()
    o_ref, _, _ = oracle.sim_ahead("pendulum", "euler", st, acts, p, spec["tau"], semantics=2, want_states=False)
    assert _close("pendulum", obs.cpu().numpy(), o_ref, torch.float32)
    with pytest.raises(RuntimeError, match=r"rc=-1\b.*bad semantics 3"):
        _native.sim_ahead(*args, 3)


def test_unknown_semantics_string():
    env, *_ = make_env("pendulum", 8, torch.float32)
    with pytest.raises(ValueError):
        env.sim_ahead_semantics = "bogus"
    assert env.sim_ahead_semantics == "ahead"
    env.sim_ahead_semantics = ACC
    assert env.sim_ahead_semantics == ACC


@pytest.mark.parametrize("env_name,dtype", [("mass_spring_damper", torch.float32), ("pendulum", torch.float64)])
def test_chained_chunks(env_name, dtype):
    """init_state = prev[2]: each chunk starts its own clock at t = 0, like one oracle call per chunk."""
    B, K = 512, 30
    env, props, keep, spec, st, acts = _problem(env_name, B, 3 * K, dtype, seed=421)
    state, ref_st = to_state(env, st), st
    for c in range(3):
        chunk = np.ascontiguousarray(acts[:, c * K:(c + 1) * K])
        obs, states, last = env.vmap_sim_ahead(state, torch.as_tensor(chunk, device=env.device), env.tau, env.tau)
        o_ref, s_ref, l_ref = oracle.sim_ahead(env_name, "euler", ref_st, chunk, props, spec["tau"],
                                               semantics=oracle.SEM_AHEAD_ACCUMULATED_T)
        assert _close(env_name, obs.cpu().numpy(), o_ref, dtype), (c, max_err(obs.cpu().numpy(), o_ref))
        state, ref_st = last, [np.asarray(x) for x in l_ref]
