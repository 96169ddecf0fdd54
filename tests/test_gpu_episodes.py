"""Episode rollouts on the GPU (`vmap_rollout_episodes`, sim_episodes_kernel), inputs E1 / E2 of tests/helpers_episodes.py:
1. replay: a host loop over launches the project already has — `vmap_gym_step` on the returned actions, `torch.where` on the returned
   `reset` with reset row e mod R — gives every observation row, state row, the last state and, on the stepped lanes, reward /
   terminated / truncated bit for bit (reset lanes: row 0 of an open-loop launch from the reset row; their gym outputs are test 3's);
2. `reset` is the rule: recomputed from the returned terminated / truncated rows, max_episode_steps, episode_steps and end_on;
   n_resets is its row sum, episode_steps the recount;
3. reward / truncated / terminated are `vmap_generate_rew_trunc_term_ahead(states, actions)` bit for bit;
4. actions from the RETURNED observation rows, reset rows included: ReLU and N0 bit for bit with the exact CPU fused multiply-add,
   tanh within helpers_policy.policy_bounds (tests/test_gpu_policy.py check_policy);
5. the independent fp64 oracle episode loop (E1): environments whose reset pattern agrees within 100 x the distance of the open-loop
   launch to oracle.sim_ahead (floor 1e-12: tests/test_gpu_feedback.py check_independent's rule); at most 2 % may disagree;
6. forms on pendulum and PMSM; 7. no episode ends: `vmap_sim_ahead_policy` bit for bit.

Measured on an MI355X: DESIGN.md §4.14."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import oracle
import helpers_episodes as he
import helpers_policy as hp
from exciting_environments_amd import _native
from helpers import make_env, to_state
from helpers_feedback import saturated_env
from helpers_vjp import obs_floor
from test_gpu_policy import check_policy

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float64]
DTYPE_IDS = ["fp32", "fp64"]
MAIN = [(c, a) for c in ("E1", "E2") for a in hp.ACTIVATIONS]
MAIN_IDS = [f"{c}-{a}" for c, a in MAIN]


def _dev(x, env, dtype=None):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=dtype or env.dtype, device=env.device)


def rollout(env, inp, activation, K=he.K, end_on=he.END_BOTH, max_episode_steps=None, steps_in="inp", reset_states=None, noise=True,
            clip=hp.CLIP):
    """One vmap_rollout_episodes call -> dict of what it returned (+ what it started from, and the reset rows as States)"""
    control = inp.get("control")
    state = to_state(env, inp["st"], reference=inp["refs"] if control else None)
    rows = [to_state(env, r, reference=inp["refs"] if control else None) for r in inp["reset"]]
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], activation)
    nz = None
    if noise:
        nz = env.new_actions_buffer(K)
        nz.copy_(_dev(inp["noise"][:, :K], env))
    steps = inp["steps_in"] if isinstance(steps_in, str) else steps_in
    mx = inp["max_episode_steps"] if max_episode_steps is None else max_episode_steps
    r = env.vmap_rollout_episodes(state, policy, K, inp["tau"], rows if reset_states is None else reset_states, noise=nz, clip=clip,
                                  end_on=end_on, max_episode_steps=mx, episode_steps=None if steps is None else _dev(steps, env, torch.int32))
    assert env.last_policy_launch == "sim_episodes_kernel" and _native.last_launch() == "sim_episodes_kernel"
    B, OW, A, TW = env.batch_size, env._obs_dim(), env.action_dim, _native.truncated_width(env.ENV_ID, len(env.control_state))
    assert tuple(r.observations.shape) == (B, K + 1, OW) and tuple(r.actions.shape) == (B, K, A)
    assert tuple(r.reward.shape) == (B, K) and r.reward.dtype == env.dtype
    assert tuple(r.terminated.shape) == tuple(r.reset.shape) == (B, K) and r.terminated.dtype == r.reset.dtype == torch.bool
    assert tuple(r.truncated.shape) == (B, K + 1, TW) and r.truncated.dtype == torch.bool
    assert tuple(r.n_resets.shape) == tuple(r.episode_steps.shape) == (B,) and r.n_resets.dtype == torch.int32
    if B > 1 and K > 0:  # zero-copy views of lane-major memory
        assert tuple(r.observations.stride()) == (1, OW * B, B) and tuple(r.reward.stride()) == (1, B) and tuple(r.reset.stride()) == (1, B)
        assert tuple(r.truncated.stride()) == (TW, B * TW, 1)
    return dict(env=env, state=state, rows=rows, r=r, obs=r.observations, actions=r.actions, K=K, sub=1, tau=inp["tau"], activation=activation,
                noise=noise, clip=clip, end_on=end_on, max_episode_steps=mx, steps_in=np.zeros(B, np.int32) if steps is None else np.asarray(steps))


@functools.lru_cache(maxsize=None)
def main_run(env_name, deadtime, solver, dtype, case, activation):
    spec, inp = he.main_case(env_name, deadtime, case)
    inp = dict(inp, tau=spec["tau"])
    env, _, _, _ = make_env(env_name, he.B, dtype, solver, spec=spec, control_state=he.CONTROL[env_name])
    return rollout(env, inp, activation), inp, spec


def _row0(env, states, actions):
    """terminated of row 0 from a launch the project already has: the gym outputs of the two-row trajectory (row 0, row 0)"""
    two = lambda tree: env.PhysicalState(**{n: getattr(tree, n)[:, [0, 0]] for n in env.STATE_FIELDS})
    tree = replace(states, physical_state=two(states.physical_state), reference=two(states.reference))
    _, _, term = env.vmap_generate_rew_trunc_term_ahead(tree, actions[:, :1])
    return term.reshape(-1)


def _observe(env, state, tau):
    """The observation row of a state as the trajectory kernels save it: row 0 of an open-loop launch without an action"""
    keep = env.sim_ahead_semantics
    env.sim_ahead_semantics = "step"
    try:
        obs, _, _ = env.vmap_sim_ahead(state, torch.zeros((env.batch_size, 0, env.action_dim), dtype=env.dtype, device=env.device), tau, tau)
    finally:
        env.sim_ahead_semantics = keep
    return obs[:, 0].clone()


def check_replay(run):
    """Test 1 on one run"""
    env, r, K = run["env"], run["r"], run["K"]
    B, R = env.batch_size, len(run["rows"])
    fields = env.STATE_FIELDS
    row_obs = [_observe(env, s, run["tau"]) for s in run["rows"]]
    state = run["state"]
    e = torch.zeros(B, dtype=torch.int64, device=env.device)
    assert torch.equal(r.observations[:, 0], _observe(env, state, run["tau"]))
    for n in range(K):
        if r.states is not None:
            for f in fields:
                assert torch.equal(getattr(r.states.physical_state, f)[:, n], getattr(state.physical_state, f)), (n, f)
        obs, rew, term, trunc, stepped = env.vmap_gym_step(state, r.actions[:, n].contiguous())
        end = r.reset[:, n]
        pick = e % R
        for f in fields:
            leaf = getattr(stepped.physical_state, f)
            for j in range(R):
                leaf = torch.where(end & (pick == j), getattr(run["rows"][j].physical_state, f), leaf)
            setattr(stepped.physical_state, f, leaf)
        for j in range(R):
            obs = torch.where((end & (pick == j))[:, None], row_obs[j], obs)
        assert torch.equal(r.observations[:, n + 1], obs), (n, int((r.observations[:, n + 1] != obs).any(dim=1).sum()))
        keep = ~end
        assert torch.equal(r.reward[:, n][keep], rew.reshape(-1)[keep]), n
        assert torch.equal(r.terminated[:, n][keep], term.reshape(-1)[keep]), n
        assert torch.equal(r.truncated[:, n + 1][keep], trunc[keep]), n
        e = e + end
        state = stepped
    for f in fields:
        assert torch.equal(getattr(r.last_state.physical_state, f), getattr(state.physical_state, f)), f
        if r.states is not None:
            assert torch.equal(getattr(r.states.physical_state, f)[:, K], getattr(state.physical_state, f)), f
    assert torch.equal(r.n_resets.to(torch.int64), e)


def check_rule(run):
    """Test 2 on one run (needs the state trajectory for row 0's terminated)"""
    env, r, K = run["env"], run["r"], run["K"]
    term0 = _row0(env, r.states, r.actions).cpu().numpy() if K > 0 else np.zeros((env.batch_size,), bool)
    term = r.terminated.cpu().numpy()
    trunc = r.truncated.cpu().numpy()
    term_rows = np.concatenate([term0[:, None], term[:, :-1]], axis=1) if K > 0 else term
    reset, n, t_out, _ = he.reset_rule_np(term_rows, trunc[:, :K].any(axis=2), run["steps_in"], run["max_episode_steps"], run["end_on"])
    assert (r.reset.cpu().numpy() == reset).all(), int((r.reset.cpu().numpy() != reset).sum())
    assert (r.n_resets.cpu().numpy() == n).all() and (r.n_resets.cpu().numpy() == r.reset.sum(dim=1).cpu().numpy()).all()
    assert (r.episode_steps.cpu().numpy() == t_out).all()
    return reset


def check_gym(run):
    """Test 3 on one run"""
    env, r = run["env"], run["r"]
    rew, trunc, term = env.vmap_generate_rew_trunc_term_ahead(r.states, r.actions)
    assert torch.equal(rew.reshape(r.reward.shape), r.reward)
    assert torch.equal(trunc, r.truncated)
    assert torch.equal(term.reshape(r.terminated.shape), r.terminated)


@pytest.mark.parametrize("case,activation", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_replay_by_existing_launches_bit_for_bit(env_name, deadtime, solver, dtype, case, activation):
    run, _, _ = main_run(env_name, deadtime, solver, dtype, case, activation)
    check_replay(run)


@pytest.mark.parametrize("case,activation", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_reset_is_the_rule(env_name, deadtime, solver, dtype, case, activation):
    run, _, _ = main_run(env_name, deadtime, solver, dtype, case, activation)
    reset = check_rule(run)
    assert 0 < reset.mean() < 0.5


@pytest.mark.parametrize("case,activation", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_gym_outputs_are_functions_of_the_rows(env_name, deadtime, solver, dtype, case, activation):
    run, _, _ = main_run(env_name, deadtime, solver, dtype, case, activation)
    check_gym(run)


@pytest.mark.parametrize("case,activation", MAIN, ids=MAIN_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_actions_are_the_policy_on_the_returned_rows(env_name, deadtime, solver, dtype, case, activation):
    run, inp, _ = main_run(env_name, deadtime, solver, dtype, case, activation)
    check_policy(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", [("pendulum", None), ("pmsm", 1)])
def test_actions_without_a_hidden_layer_bit_for_bit(env_name, deadtime, dtype):
    spec = he.case_spec(env_name, deadtime)
    inp = dict(he.episode_inputs(env_name, spec, "E1", hidden=hp.NETS["N0"]), tau=spec["tau"])
    env, _, _, _ = make_env(env_name, he.B, dtype, "euler", spec=spec, control_state=he.CONTROL[env_name])
    run = rollout(env, inp, "relu")
    check_policy(run, inp)
    check_replay(run)


# ---- 5. the independent fp64 loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_independent_fp64_episode_loop(env_name, deadtime, solver, activation):
    run, inp, spec = main_run(env_name, deadtime, solver, torch.float64, "E1", activation)
    want = he.oracle_case(env_name, deadtime, solver, "E1", activation)
    env, r = run["env"], run["r"]
    agree = (r.reset.cpu().numpy() == want["reset"]).all(axis=1)
    share = 1.0 - float(agree.mean())
    # the project's rule: 100 x the open-loop launch's distance to oracle.sim_ahead on the same actions, floor 1e-12
    keep = env.sim_ahead_semantics, env.launch_opts
    env.sim_ahead_semantics, env.launch_opts = "step", _native.launch_opts(envs_per_lane=1)
    try:
        open_gpu, _, _ = env.vmap_sim_ahead(run["state"], r.actions, run["tau"], run["tau"])
    finally:
        env.sim_ahead_semantics, env.launch_opts = keep
    acts = r.actions.cpu().numpy()
    props, _keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, he.B)
    open_obs, _, _ = oracle.sim_ahead(env_name, solver, inp["st"], acts, props, spec["tau"], semantics=oracle.SEM_STEP, control=he._ctl(inp))
    d_open = obs_floor(open_gpu.cpu().numpy(), open_obs, env_name)
    tol = max(100.0 * d_open, 1e-12)
    got = r.observations.cpu().numpy()
    d_obs = obs_floor(got[agree], want["obs"][agree], env_name)
    d_act = float(np.max(np.abs(acts[agree] - want["actions"][agree]), initial=0.0))
    d_rew = float(np.max(np.abs(r.reward.cpu().numpy()[agree] - want["reward"][agree]), initial=0.0))
    print(f"fp64 {env_name} deadtime {deadtime} {solver} {activation}: reset pattern disagrees in {share:.4f} of the environments; open loop "
          f"vs oracle {d_open:.3e}, episodes vs oracle {d_obs:.3e}, actions {d_act:.3e}, reward {d_rew:.3e}, allowed {tol:.3e}")
    assert share <= 0.02
    assert d_obs <= tol and d_act <= tol
    assert (r.n_resets.cpu().numpy()[agree] == want["n_resets"][agree]).all()
    assert (r.episode_steps.cpu().numpy()[agree] == want["steps_out"][agree]).all()


# ---- 6. forms ------------------------------------------------------------------------------------------------------------------------
FORM_CASES = [("pendulum", None), ("pmsm", 1)]


def _form(env_name, deadtime, dtype, B=he.B, K=he.K, control="default", hidden=None, n_rows=he.R, case="E1", per_env_props=False, solver="euler"):
    spec = he.case_spec(env_name, deadtime)
    if per_env_props:  # a static parameter and an action bound as [B] arrays
        rng = np.random.default_rng(9)
        pname, aname = ("l", "torque") if env_name == "pendulum" else ("r_s", "u_q")
        spec["params"][pname] = spec["params"][pname] * rng.uniform(0.8, 1.2, B)
        lo, hi = spec["act_norm"][aname]
        spec["act_norm"][aname] = (lo * rng.uniform(0.8, 1.0, B), hi * rng.uniform(0.8, 1.0, B))
    ctl = he.CONTROL[env_name] if control == "default" else control
    inp = dict(he.episode_inputs(env_name, spec, case, hidden=hidden, B=B, K=K, n_rows=n_rows, control=ctl), tau=spec["tau"])
    env, _, _, _ = make_env(env_name, B, dtype, solver, spec=spec, control_state=ctl)
    return env, inp


def _all_checks(run, inp):
    check_replay(run)
    check_gym(run)
    check_rule(run)
    check_policy(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_truncated_only_without_control_state(env_name, deadtime, dtype):
    env, inp = _form(env_name, deadtime, dtype, control=None)
    run = rollout(env, inp, "tanh", end_on=("truncated",))
    _all_checks(run, inp)
    assert 0 < float(run["r"].reset.float().mean()) < 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_terminated_without_control_state_resets_on_every_row(dtype):
    """The reference's semantics: reward 0 and terminated = (reward == 0) in every row, so row n + 1 is reset row n mod R"""
    env, inp = _form("pendulum", None, dtype, control=None, n_rows=3)
    run = rollout(env, inp, "relu", end_on=("terminated",), max_episode_steps=0)
    r = run["r"]
    assert r.reset.all() and r.terminated.all() and (r.reward == 0).all() and (r.n_resets == he.K).all() and (r.episode_steps == 0).all()
    for n in range(he.K):
        for f in env.STATE_FIELDS:
            assert torch.equal(getattr(r.states.physical_state, f)[:, n + 1], getattr(run["rows"][n % 3].physical_state, f))
    _all_checks(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_time_limit_only(env_name, deadtime, dtype):
    env, inp = _form(env_name, deadtime, dtype)
    run = rollout(env, inp, "tanh", end_on=(), max_episode_steps=4)
    want, _, _, time_only = he.reset_rule_np(np.zeros((he.B, he.K), bool), np.zeros((he.B, he.K), bool), inp["steps_in"], 4, ())
    assert (run["r"].reset.cpu().numpy() == want).all() and want.any() and (time_only == want).all()
    _all_checks(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_other_numbers_of_reset_rows_and_their_forms(env_name, deadtime, n_rows, dtype):
    env, inp = _form(env_name, deadtime, dtype, n_rows=n_rows, case="E2")
    run = rollout(env, inp, "relu")
    _all_checks(run, inp)
    # the same rows as a physical state with leaves [B, R] (laid out as [R][B] already, and not), and one row as a State
    stacked = [torch.stack([getattr(s.physical_state, f) for s in run["rows"]]) for f in env.STATE_FIELDS]
    for leaves in ([x.t() for x in stacked], [x.t().contiguous() for x in stacked]):
        tree = env.PhysicalState(**dict(zip(env.STATE_FIELDS, leaves)))
        again = rollout(env, inp, "relu", reset_states=tree)
        for a, b in zip(again["r"][3:], run["r"][3:]):
            assert torch.equal(a, b)
        assert torch.equal(again["obs"], run["obs"])
    if n_rows == 1:
        again = rollout(env, inp, "relu", reset_states=run["rows"][0])
        assert torch.equal(again["obs"], run["obs"]) and torch.equal(again["r"].reset, run["r"].reset)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_no_noise_no_clamp_no_state_trajectory_per_env_properties(env_name, deadtime, dtype):
    env, inp = _form(env_name, deadtime, dtype, per_env_props=True)
    run = rollout(env, inp, "tanh", noise=False, clip=None, steps_in=None)
    _all_checks(run, inp)
    env.store_state_trajectory = False
    bare = rollout(env, inp, "tanh", noise=False, clip=None, steps_in=None)
    assert bare["r"].states is None
    for a, b in zip(bare["r"][2:], run["r"][2:]):
        if torch.is_tensor(a):
            assert torch.equal(a, b)
    assert torch.equal(bare["obs"], run["obs"])
    check_replay(bare)


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_saturated_pmsm_refreshes_its_table_values_at_a_reset(dtype, activation):
    env, props, keep, spec = saturated_env(he.B, dtype, "euler", "cuda", control_state=he.CONTROL["pmsm"])
    inp = dict(he.episode_inputs("pmsm", spec, "E2"), tau=spec["tau"])
    run = rollout(env, inp, activation)
    assert (run["r"].n_resets >= 3).all()
    _all_checks(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_widest_network(env_name, deadtime, dtype):
    env, inp = _form(env_name, deadtime, dtype, hidden=hp.NETS["N2"])
    run = rollout(env, inp, "relu")
    _all_checks(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B,K", [(1, 9), (64, 9), (65, 9), (326, 0), (326, 1)])
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_batch_and_horizon_edges(env_name, deadtime, B, K, dtype):
    env, inp = _form(env_name, deadtime, dtype, B=B, K=K, case="E2")
    run = rollout(env, inp, "relu", K=K)
    r = run["r"]
    if K == 0:
        assert (r.n_resets == 0).all() and torch.equal(r.episode_steps.cpu(), torch.as_tensor(inp["steps_in"]))
        assert torch.equal(r.observations[:, 0], _observe(env, run["state"], inp["tau"]))
        for f in env.STATE_FIELDS:
            assert torch.equal(getattr(r.last_state.physical_state, f), getattr(run["state"].physical_state, f))
        two = env.vmap_rollout_episodes(run["state"], excenvs.MLPPolicy(inp["W"], inp["b"], "relu"), 1, inp["tau"], run["rows"], max_episode_steps=2)
        assert torch.equal(two.truncated[:, 0], r.truncated[:, 0])
    else:
        _all_checks(run, inp)


# ---- 7. no episode ends ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _never_leaves(env_name, deadtime, solver, activation):
    """The environments of helpers_policy's main case that the float64 oracle loop (one step per action) shows inside 98 % of the
    box in every row: |obs| <= 0.98 per column, PMSM also |i_dq| <= 0.98 of its limit -> their indices"""
    spec, inp = hp.main_case(env_name, deadtime, "N1")
    props, _keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, hp.B_MAIN)
    want = hp.oracle_policy_loop(env_name, solver, props, inp, spec["tau"], activation, sub=1)
    inside = (np.abs(want["obs"]) <= 0.98).all(axis=(1, 2))
    if env_name == "pmsm":
        fields = oracle.STATE_FIELDS["pmsm"]
        norm = lambda name: 2.0 * (want["states"][fields.index(name)] - spec["phys_norm"][name][0]) / (spec["phys_norm"][name][1] - spec["phys_norm"][name][0]) - 1.0
        inside &= (np.sqrt(norm("i_d") ** 2 + norm("i_q") ** 2) <= 0.98).all(axis=1)
    return np.where(inside)[0]


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_without_an_episode_end_it_is_the_policy_launch(env_name, deadtime, solver, dtype, activation):
    spec, inp = hp.main_case(env_name, deadtime, "N1")
    idx = _never_leaves(env_name, deadtime, solver, activation)
    assert len(idx) >= 16, len(idx)
    K = hp.K_MAIN
    sel = dict(inp, st=[v[idx] for v in inp["st"]], noise=inp["noise"][idx])
    env, _, _, _ = make_env(env_name, len(idx), dtype, solver, spec=spec)
    state = to_state(env, sel["st"])
    policy = excenvs.MLPPolicy(sel["W"], sel["b"], activation)
    nz = _dev(sel["noise"], env)
    obs, states, last, actions = env.vmap_sim_ahead_policy(state, policy, K, spec["tau"], spec["tau"], noise=nz)
    steps = np.random.default_rng(he.STEPS_SEED).integers(0, 12, len(idx)).astype(np.int32)
    r = env.vmap_rollout_episodes(state, policy, K, spec["tau"], state, noise=nz, end_on=("truncated",),
                                  max_episode_steps=K + 12 + 1, episode_steps=_dev(steps, env, torch.int32))
    assert not r.reset.any() and (r.n_resets == 0).all() and not r.truncated.any()
    assert torch.equal(r.episode_steps.cpu(), torch.as_tensor(steps) + K)
    assert torch.equal(r.observations, obs) and torch.equal(r.actions, actions)
    for f in env.STATE_FIELDS:
        assert torch.equal(getattr(r.states.physical_state, f), getattr(states.physical_state, f))
        assert torch.equal(getattr(r.last_state.physical_state, f), getattr(last.physical_state, f))
