"""Policy rollouts on the GPU (`vmap_sim_ahead_policy`, sim_policy_kernel):
1. dynamics: the returned actions fed to the open-loop `vmap_sim_ahead` ("step" semantics, one environment per lane) give the same
   observations, state rows and last state bit for bit — every case, solver and dtype with the network N1 and both activations, and
   the saturated PMSM;
2. policy, from the RETURNED observation rows: (a) ReLU networks and N0: the actions bit for bit the contract evaluated with an exact
   CPU fused multiply-add (helpers_policy.fma_exact), every environment; (b) tanh networks: every action entry within the forward
   bound of helpers_policy.policy_bounds and nothing more; (c) the device's tanh within 5 ulp of float64 numpy's (asserted as
   10 u |tanh|) through a network whose every multiply-add is exact, from |x| ~ 1e-13 to beyond the overflow of exp(2 x);
3. the independent fp64 closed loop (numpy policy over oracle.step) within 100 x the distance the open-loop launch shows against
   oracle.sim_ahead on the same actions (floor 1e-12 of full scale): tests/test_gpu_feedback.py check_independent's rule;
4. forms: N2, N0 and N3, per-environment properties, control columns fed into the network, no noise, no clamp, a plain noise tensor,
   no state trajectory, K = 1, B = 1, K = 0, B = 64 exactly;
5. all-zero parameters, no clamp: the open-loop launch on the noise tensor, bit for bit;
6. `MLPPolicy.from_torch`: the torch module's float64 forward on the returned observation rows within bound (b) of the actions;
7. `policy.params` updated in place between two launches (same stream, and on a side stream between two wait_stream calls): the next
   launch computes with the new values, bit for bit.

Measured on an MI355X (largest error / bound of 2b; distances of 3): see DESIGN.md §4.13."""
import functools

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import oracle
import helpers_policy as hp
from exciting_environments_amd import _native
from helpers import NP_DTYPE, make_env, to_state
from helpers_feedback import saturated_env
from helpers_vjp import obs_floor

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float64]
DTYPE_IDS = ["fp32", "fp64"]


def _dev(x, env):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=env.dtype, device=env.device)


def _as_seen(inp, dtype):
    """The inputs as the kernel sees them: rounded to the working dtype, as float64"""
    npdt = NP_DTYPE[dtype]
    r = lambda v: None if v is None else np.asarray(v).astype(npdt).astype(np.float64)
    out = dict(W=[r(w) for w in inp["W"]], b=[r(b) for b in inp["b"]], noise=r(inp["noise"]), st=[r(v) for v in inp["st"]])
    out["refs"] = None if inp.get("refs") is None else {n: r(v) for n, v in inp["refs"].items()}
    return out


def rollout(env, inp, activation, K, sub, tau, clip=hp.CLIP, control=None, noise=True, plain_noise=False):
    """One vmap_sim_ahead_policy call -> dict of what it returned (+ the state it started from)"""
    state = to_state(env, inp["st"], reference=inp["refs"] if control else None)
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], activation)
    nz = _dev(inp["noise"], env) if noise else None
    if nz is not None and not plain_noise:  # a lane-major view: read in place
        buf = env.new_actions_buffer(K)
        buf.copy_(nz)
        nz = buf
    obs, states, last, actions = env.vmap_sim_ahead_policy(state, policy, K, tau, tau * sub, noise=nz, clip=clip)
    assert env.last_policy_launch == "sim_policy_kernel" and _native.last_launch() == "sim_policy_kernel"
    B, OW, A, N = env.batch_size, env._obs_dim(), env.action_dim, K * sub
    assert tuple(obs.shape) == (B, N + 1, OW) and tuple(actions.shape) == (B, K, A) and obs.grad_fn is None and actions.grad_fn is None
    assert tuple(obs.stride()) == (1, OW * B, B) or B == 1
    return dict(env=env, state=state, obs=obs, states=states, last=last, actions=actions, K=K, sub=sub, tau=tau, activation=activation,
                noise=noise, clip=clip)


def check_dynamics(run):
    """Test 1 on one run: the open-loop kernel of the parent commit on the returned actions, bit for bit"""
    env = run["env"]
    keep = env.sim_ahead_semantics, env.launch_opts
    env.sim_ahead_semantics, env.launch_opts = "step", _native.launch_opts(envs_per_lane=1)
    try:
        obs, states, last = env.vmap_sim_ahead(run["state"], run["actions"], run["tau"], run["tau"] * run["sub"])
        launch = _native.last_launch()
    finally:
        env.sim_ahead_semantics, env.launch_opts = keep
    assert "sim_ahead_kernel" in launch, launch
    assert torch.equal(obs, run["obs"]), float((obs - run["obs"]).abs().max())
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(last.physical_state, n), getattr(run["last"].physical_state, n)), n
        if run["states"] is not None:
            assert torch.equal(getattr(states.physical_state, n), getattr(run["states"].physical_state, n)), n


def check_exact(run, inp):
    """Test 2a on one run (ReLU or no hidden layer): the actions bit for bit from the returned observation rows"""
    env = run["env"]
    npdt = NP_DTYPE[env.dtype]
    seen = _as_seen(inp, env.dtype)
    K, sub = run["K"], run["sub"]
    obs = run["obs"].cpu().numpy()
    got = run["actions"].cpu().numpy()
    assert obs.dtype == npdt and got.dtype == npdt
    for k in range(K):
        want, _, _ = hp.mlp_np(obs[:, k * sub], seen["W"], seen["b"], "relu", seen["noise"][:, k] if run["noise"] else None, run["clip"],
                               exact=npdt)
        assert want.dtype == npdt
        same = want.view(np.int32 if npdt is np.float32 else np.int64) == got[:, k].view(np.int32 if npdt is np.float32 else np.int64)
        assert same.all(), (k, int((~same).sum()), float(np.max(np.abs(want.astype(np.float64) - got[:, k]))))


def check_bound(run, inp, W=None, b=None):
    """Test 2b on one run: every action entry within the forward bound, from the returned observation rows -> largest error / bound"""
    env = run["env"]
    seen = _as_seen(inp, env.dtype)
    K, sub = run["K"], run["sub"]
    obs = run["obs"].cpu().numpy().astype(np.float64)
    want, bound = hp.policy_bounds(obs[:, 0:K * sub:sub], seen["W"] if W is None else W, seen["b"] if b is None else b, run["activation"],
                                   seen["noise"] if run["noise"] else None, run["clip"], NP_DTYPE[env.dtype])
    got = run["actions"].cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"policy: largest error / bound {worst:.3f} (largest error {float(err.max()) if err.size else 0.0:.3e})")
    assert np.all(err <= bound), worst
    return worst


def check_policy(run, inp):
    if run["activation"] == "relu" or len(inp["W"]) == 1:
        check_exact(run, inp)
    else:
        check_bound(run, inp)


@functools.lru_cache(maxsize=None)
def main_run(env_name, deadtime, solver, dtype, activation):
    spec, inp = hp.main_case(env_name, deadtime, "N1")
    env, _, _, _ = make_env(env_name, hp.B_MAIN, dtype, solver, spec=spec)
    return rollout(env, inp, activation, hp.K_MAIN, hp.substeps_of(env_name), spec["tau"]), inp, spec


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_dynamics_are_the_open_loop_kernels_bit_for_bit(env_name, deadtime, solver, dtype, activation):
    run, _, _ = main_run(env_name, deadtime, solver, dtype, activation)
    check_dynamics(run)
    assert bool(torch.isfinite(run["obs"]).all())
    share = float((run["actions"].abs() >= 1.0).float().mean())
    assert 0.05 < share < 0.6, share  # the clamp is at work in this run too


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_relu_actions_are_the_contract_bit_for_bit(env_name, deadtime, solver, dtype):
    run, inp, _ = main_run(env_name, deadtime, solver, dtype, "relu")
    check_exact(run, inp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_tanh_actions_lie_within_the_forward_bound(env_name, deadtime, solver, dtype):
    run, inp, _ = main_run(env_name, deadtime, solver, dtype, "tanh")
    check_bound(run, inp)


TANH_REACH = {2.0 ** 7: 44.0, 2.0 ** 9: 355.0}  # where exp(2 x) overflows in fp32 / fp64: a tanh built on it goes wrong beyond


@pytest.mark.parametrize("scale", [4.0, 2.0 ** -10, 2.0 ** 7, 2.0 ** 9, 2.0 ** -40], ids=["s=4", "s=2^-10", "s=2^7", "s=2^9", "s=2^-40"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", [("pendulum", None), ("pmsm", 1)])
def test_the_device_tanh_is_within_five_ulp(env_name, deadtime, dtype, scale):
    """OW -> OW -> A with W_1 = s I, b = 0, W_2 one-hot, no noise, no clamp: every fma is exact, so a[q] = tanh_device(s obs[q]).
    Each entry within 5 ulp of float64 np.tanh, asserted as 10 u |tanh|: the feature's requirement (OpenCL's conformance bound).
    s = 2^7 and 2^9 reach |x| > 44 and > 355, where exp(2 x) overflows in fp32 and fp64; s = 2^-40 the linear end (the products are
    normal numbers in both formats). No NaN, no inf, |a| <= 1 at every scale."""
    spec = hp.case_spec(env_name, deadtime)
    env, _, _, _ = make_env(env_name, hp.B_MAIN, dtype, "euler", spec=spec)
    OW, A = env._obs_dim(), env.action_dim
    inp = hp.policy_inputs(env_name, spec, (OW,))
    inp["W"] = [scale * np.eye(OW), np.eye(A, OW)]
    inp["b"] = [np.zeros(OW), np.zeros(A)]
    run = rollout(env, inp, "tanh", hp.K_MAIN, hp.substeps_of(env_name), spec["tau"], clip=None, noise=False)
    sub = run["sub"]
    x = run["obs"].cpu().numpy().astype(np.float64)[:, 0:hp.K_MAIN * sub:sub, :A]
    want = np.tanh(scale * x)
    got = run["actions"].cpu().numpy().astype(np.float64)
    u = hp.U[np.dtype(NP_DTYPE[dtype])]
    err = np.abs(got - want)
    print(f"tanh({scale} x): largest error {float(np.max(err / np.maximum(u * np.abs(want), 1e-300))):.2f} u |tanh|, "
          f"|x| up to {float(np.abs(scale * x).max()):.3g}")
    assert np.all(err <= 10.0 * u * np.abs(want))
    assert np.any(want != 0)
    assert np.isfinite(got).all() and float(np.abs(got).max()) <= 1.0
    if scale in TANH_REACH:
        assert float(np.abs(scale * x).max()) > TANH_REACH[scale], float(np.abs(scale * x).max())
    check_dynamics(run)


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_independent_closed_loop_in_fp64(env_name, deadtime, solver, activation):
    """Tolerance: 100 x the distance of the open-loop fp64 launch (== the closed-loop rows, test 1) from oracle.sim_ahead on the
    same actions, at least 1e-12 of full scale. The margin is for numpy's unfused multiply-adds (and its tanh) in the policy and
    their amplification over the 7 action rows. Distances are relative to the largest magnitude, wrapped angles on the circle."""
    run, inp, spec = main_run(env_name, deadtime, solver, torch.float64, activation)
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, hp.B_MAIN)
    check_independent(run, inp, props, hp.oracle_case(env_name, deadtime, solver, "N1", activation), env_name, solver, spec["tau"],
                      f"fp64 {env_name} deadtime {deadtime} {solver} {activation}")


def check_independent(run, inp, props, want, env_name, solver, tau, label, control=None):
    """Test 3 on one fp64 run: observations and actions against the oracle loop `want`, within the measured tolerance -> the largest
    distance / tolerance. control: the controlled fields, whose references inp["refs"] the open-loop oracle shows too."""
    got_obs = run["obs"].cpu().numpy()
    acts = run["actions"].cpu().numpy()
    ctl = [(n, inp["refs"][n]) for n in control] if control else None
    open_obs, _, _ = oracle.sim_ahead(env_name, solver, inp["st"], acts, props, tau, substeps=run["sub"], semantics=oracle.SEM_STEP, control=ctl)
    d_open = obs_floor(got_obs, open_obs, env_name)
    d_closed = obs_floor(got_obs, want["obs"], env_name)
    d_act = float(np.max(np.abs(acts - want["actions"]), initial=0.0))
    tol = max(100.0 * d_open, 1e-12)
    print(f"{label}: open loop vs oracle {d_open:.3e}, closed loop vs oracle {d_closed:.3e}, actions {d_act:.3e}, allowed {tol:.3e}")
    assert d_closed <= tol and d_act <= tol
    return max(d_closed, d_act) / tol


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_saturated_pmsm(dtype, activation):
    env, props, keep, spec = saturated_env(hp.B_MAIN, dtype, "euler", "cuda")
    inp = hp.policy_inputs("pmsm", spec, hp.NETS["N1"])
    run = rollout(env, inp, activation, hp.K_MAIN, 1, spec["tau"])
    check_dynamics(run)
    check_policy(run, inp)
    if dtype is torch.float64:
        want = hp.oracle_policy_loop("pmsm", "euler", props, inp, spec["tau"], activation)
        check_independent(run, inp, props, want, "pmsm", "euler", spec["tau"], f"fp64 saturated PMSM euler {activation}")


# ---- 4. forms -------------------------------------------------------------------------------------------------------------------------
FORM_CASES = [("pendulum", None), ("pmsm", 1)]
CONTROL = {"pendulum": ["theta", "omega"], "pmsm": ["i_d", "i_q"]}


def _form_env(env_name, deadtime, dtype, B=hp.B_MAIN, control=None, per_env_props=False):
    spec = hp.case_spec(env_name, deadtime)
    if per_env_props:  # a static parameter and an action bound as [B] arrays
        rng = np.random.default_rng(9)
        pname, aname = ("l", "torque") if env_name == "pendulum" else ("r_s", "u_q")
        spec["params"][pname] = spec["params"][pname] * rng.uniform(0.8, 1.2, B)
        lo, hi = spec["act_norm"][aname]
        spec["act_norm"][aname] = (lo, hi * rng.uniform(0.7, 1.0, B))
    env, _, _, _ = make_env(env_name, B, dtype, "euler", spec=spec, control_state=control)
    return env, spec


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("net", ["N2", "N0", "N3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_widest_deepest_and_smallest_networks(env_name, deadtime, dtype, net, activation):
    env, spec = _form_env(env_name, deadtime, dtype)
    inp = hp.policy_inputs(env_name, spec, hp.NETS[net])
    run = rollout(env, inp, activation, hp.K_MAIN, hp.substeps_of(env_name), spec["tau"])
    check_dynamics(run)
    check_policy(run, inp)


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_per_environment_properties(env_name, deadtime, dtype, activation):
    env, spec = _form_env(env_name, deadtime, dtype, per_env_props=True)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    run = rollout(env, inp, activation, hp.K_MAIN, hp.substeps_of(env_name), spec["tau"])
    check_dynamics(run)
    check_policy(run, inp)


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_reference_columns_are_fed_into_the_network(env_name, deadtime, dtype, activation):
    control = CONTROL[env_name]
    env, spec = _form_env(env_name, deadtime, dtype, control=control)
    O = hp.obs_width(env_name)
    for net in ("N1", "N0"):
        inp = hp.policy_inputs(env_name, spec, hp.NETS[net], control=control)
        assert env._obs_dim() == O + 2 and inp["widths"][0] == O + 2
        run = rollout(env, inp, activation, hp.K_MAIN, hp.substeps_of(env_name), spec["tau"], control=control)
        check_dynamics(run)
        check_policy(run, inp)
        # the columns hold the normalised references, and their weights matter
        for j, name in enumerate(control):
            lo, hi = spec["phys_norm"][name]
            want = 2 * (_as_seen(inp, dtype)["refs"][name] - lo) / (hi - lo) - 1
            np.testing.assert_allclose(run["obs"][:, :, O + j].cpu().numpy(), np.repeat(want[:, None], run["obs"].shape[1], 1),
                                       rtol=0, atol=4 * hp.U[np.dtype(NP_DTYPE[dtype])] * 4)
        blind = dict(inp, W=[w.copy() for w in inp["W"]])
        blind["W"][0][:, O:] = 0.0
        other = rollout(env, blind, activation, hp.K_MAIN, hp.substeps_of(env_name), spec["tau"], control=control)
        assert not torch.equal(other["actions"], run["actions"])


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_without_noise_and_without_clamp(env_name, deadtime, dtype, activation):
    env, spec = _form_env(env_name, deadtime, dtype)
    sub = hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    for noise, clip in ((False, hp.CLIP), (True, None), (False, None), (True, (-0.25, 0.5))):
        run = rollout(env, inp, activation, hp.K_MAIN, sub, spec["tau"], clip=clip, noise=noise)
        check_dynamics(run)
        check_policy(run, inp)
        if clip is None and noise:
            assert float(run["actions"].abs().max()) > 1.0
        if clip == (-0.25, 0.5):
            assert float(run["actions"].min()) == -0.25 and float(run["actions"].max()) == 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_plain_noise_tensor_and_no_state_trajectory(env_name, deadtime, dtype):
    env, spec = _form_env(env_name, deadtime, dtype)
    sub = hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    ref = rollout(env, inp, "tanh", hp.K_MAIN, sub, spec["tau"])
    plain = rollout(env, inp, "tanh", hp.K_MAIN, sub, spec["tau"], plain_noise=True)  # a contiguous [B, K, A] tensor: copied lane-major
    assert torch.equal(plain["obs"], ref["obs"]) and torch.equal(plain["actions"], ref["actions"])
    check_dynamics(plain)
    check_policy(plain, inp)
    env.store_state_trajectory = False  # state_traj == NULL at the C level
    bare = rollout(env, inp, "tanh", hp.K_MAIN, sub, spec["tau"])
    assert bare["states"] is None
    assert torch.equal(bare["obs"], ref["obs"]) and torch.equal(bare["actions"], ref["actions"])
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(bare["last"].physical_state, n), getattr(ref["last"].physical_state, n)), n
        assert torch.equal(getattr(ref["last"].physical_state, n), getattr(ref["states"].physical_state, n)[:, -1]), n
    check_dynamics(bare)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("B,K", [(hp.B_MAIN, 1), (1, hp.K_MAIN), (1, 1), (hp.B_MAIN, 0), (64, hp.K_MAIN)])
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_single_rows_single_environments_and_one_full_wavefront(env_name, deadtime, B, K, dtype):
    env, spec = _form_env(env_name, deadtime, dtype, B=B)
    for activation in hp.ACTIVATIONS:
        inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"], B=B, K=K)
        run = rollout(env, inp, activation, K, hp.substeps_of(env_name), spec["tau"])
        check_policy(run, inp)
        if K > 0:
            check_dynamics(run)
        else:  # row 0 only: the first row of any longer run; the state passes through
            assert run["obs"].shape[1] == 1 and run["actions"].shape[1] == 0
            longer = rollout(env, hp.policy_inputs(env_name, spec, hp.NETS["N1"], B=B, K=1), activation, 1, hp.substeps_of(env_name), spec["tau"])
            assert torch.equal(run["obs"], longer["obs"][:, :1])
            for n, v in zip(env.STATE_FIELDS, inp["st"]):
                assert torch.equal(getattr(run["last"].physical_state, n), _dev(v, env)), n


# ---- 5. open loop as a special case -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["N1", "N0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES + [("cartpole", None)])
def test_zero_parameters_are_the_open_loop_launch(env_name, deadtime, dtype, net):
    env, spec = _form_env(env_name, deadtime, dtype)
    sub = hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS[net])
    inp["W"] = [np.zeros_like(w) for w in inp["W"]]
    inp["b"] = [np.zeros_like(b) for b in inp["b"]]
    run = rollout(env, inp, "tanh", hp.K_MAIN, sub, spec["tau"], clip=None)  # noise reaches beyond [-1, 1]: nothing clamps
    acts = _dev(inp["noise"], env)
    assert torch.equal(run["actions"], acts)
    env.sim_ahead_semantics = "step"
    obs, states, last = env.vmap_sim_ahead(to_state(env, inp["st"]), acts, spec["tau"], spec["tau"] * sub)  # the default plan
    assert torch.equal(obs, run["obs"])
    for n in env.STATE_FIELDS:
        assert torch.equal(getattr(states.physical_state, n), getattr(run["states"].physical_state, n)), n
        assert torch.equal(getattr(last.physical_state, n), getattr(run["last"].physical_state, n)), n


# ---- 6. a torch module as the policy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_a_torch_module_is_the_policy(env_name, deadtime, dtype, activation):
    env, spec = _form_env(env_name, deadtime, dtype)
    sub = hp.substeps_of(env_name)
    OW, A = env._obs_dim(), env.action_dim
    nn = torch.nn
    act = nn.Tanh if activation == "tanh" else nn.ReLU
    torch.manual_seed(17)
    module = nn.Sequential(nn.Linear(OW, 11), act(), nn.Linear(11, 5), act(), nn.Linear(5, A)).to(dtype)
    policy = excenvs.MLPPolicy.from_torch(module)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    noise = _dev(inp["noise"], env)
    obs, states, last, actions = env.vmap_sim_ahead_policy(to_state(env, inp["st"]), policy, None, spec["tau"], spec["tau"] * sub, noise=noise)
    assert env.last_policy_launch == "sim_policy_kernel" and actions.shape == (hp.B_MAIN, hp.K_MAIN, A)
    rows = obs[:, 0:hp.K_MAIN * sub:sub].cpu().double()
    with torch.no_grad():
        y = module.double()(rows)
    nz = noise.cpu().double()
    want = torch.clamp(nz + y, -1.0, 1.0).numpy()
    W = [m.weight.detach().numpy() for m in module if isinstance(m, nn.Linear)]
    b = [m.bias.detach().numpy() for m in module if isinstance(m, nn.Linear)]
    mine, bound = hp.policy_bounds(rows.numpy(), W, b, activation, nz.numpy(), hp.CLIP, NP_DTYPE[dtype])
    err = np.abs(actions.cpu().numpy().astype(np.float64) - want)
    print(f"torch module: largest error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)
    assert np.all(np.abs(mine - want) <= bound)  # torch's float64 forward and the restatement: the same function


# ---- 7. the parameters are read in place -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_stream", [False, True], ids=["same_stream", "side_stream"])
@pytest.mark.parametrize("net", ["N1", "N2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("env_name,deadtime", FORM_CASES)
def test_parameters_updated_in_place_are_the_next_launchs(env_name, deadtime, dtype, net, side_stream):
    """A training loop updates `policy.params` in place between launches. The policy is built on the environment's device in its
    dtype, so the kernel's scalar loads read `policy.params` itself. Roll out, `policy.params.copy_(second set)`, roll out again with
    no synchronisation in between: the second run's actions are the contract on the SECOND set bit for bit (check_exact), the bits of a
    fresh MLPPolicy built from the second set, and not the first run's. side_stream: the update is enqueued on a second stream
    between two `wait_stream` calls, INTEGRATION.md's stream discipline, nothing more."""
    env, spec = _form_env(env_name, deadtime, dtype)
    sub = hp.substeps_of(env_name)
    first = hp.policy_inputs(env_name, spec, hp.NETS[net])
    other = hp.policy_inputs(env_name, spec, hp.NETS[net], seed=hp.SEED + 1)
    second = dict(first, W=other["W"], b=other["b"])  # the same states and noise under the second parameter set
    policy = excenvs.MLPPolicy(first["W"], first["b"], "relu", device=env.device, dtype=dtype)
    assert policy.on(env.device, dtype).data_ptr() == policy.params.data_ptr()
    fresh = excenvs.MLPPolicy(second["W"], second["b"], "relu", device=env.device, dtype=dtype)
    new_params = fresh.params.clone()
    state = to_state(env, first["st"])
    noise = env.new_actions_buffer(hp.K_MAIN)
    noise.copy_(_dev(first["noise"], env))
    launch = lambda p: env.vmap_sim_ahead_policy(state, p, hp.K_MAIN, spec["tau"], spec["tau"] * sub, noise=noise)
    obs1, _, _, act1 = launch(policy)
    if side_stream:
        main, side = torch.cuda.current_stream(), torch.cuda.Stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            policy.params.copy_(new_params)
        main.wait_stream(side)
    else:
        policy.params.copy_(new_params)
    obs2, states2, last2, act2 = launch(policy)
    assert policy.on(env.device, dtype).data_ptr() == policy.params.data_ptr()
    obs3, _, _, act3 = launch(fresh)
    torch.cuda.synchronize()
    run = dict(env=env, state=state, obs=obs2, states=states2, last=last2, actions=act2, K=hp.K_MAIN, sub=sub, tau=spec["tau"],
               activation="relu", noise=True, clip=hp.CLIP)
    check_exact(run, second)
    assert torch.equal(act2, act3) and torch.equal(obs2, obs3)
    assert not torch.equal(act2, act1)
    print(f"in-place update {env_name} {dtype} {net} {'side stream' if side_stream else 'same stream'}: second run == the fresh "
          f"policy's bits; differs from the first run in {float((act2 != act1).float().mean()):.3f} of the action entries")
