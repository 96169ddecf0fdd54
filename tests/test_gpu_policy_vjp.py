"""Reverse mode of the policy rollout on the GPU (`vmap_sim_ahead_policy_vjp`, `vmap_sim_ahead_policy(differentiable=True)`;
sim_policy_vjp_kernel and the parameter contraction in torch):
1. fp64 against the float64 torch twin (helpers_policy_vjp): every model, three solvers, network N1 with both activations, the other
   networks on pendulum and PMSM; four cotangent groups (the last one, grad_actions alone, reaches the initial state only through
   the transposed network); grad_state0, grad_noise and grad_params within 1e-8 of the tensor's largest magnitude;
2. fp32: within 32 x the forward floor, the rule of tests/test_gpu_feedback_vjp.py, environments inside the margins excluded;
3. bit-for-bit equalities: all-zero weights are the open-loop reverse kernel on the returned actions, two calls agree, the recording
   form gives the explicit form's bits;
4. against the parent commit's only route: a chain of differentiable vmap_step calls with the network in torch, 2e-8;
5. a directional finite difference through the real forward launch, 1e-6 of the largest derivative;
6. the episode mask on what vmap_rollout_episodes returned, against the twin with torch.where on the same mask;
7. forms: no noise, no clamp, control columns, absent cotangent groups, K = 1 and 0, B = 1, 64 and 65, param_grads=False.
Every case prints its figures."""
import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_policy as hp
import helpers_policy_vjp as hv
from exciting_environments_amd import _native
from helpers import NP_DTYPE, make_env, to_state
from helpers_vjp import KINK_CAP, KINK_MARGIN, Twin, case_spec, obs_floor, rel_dist

pytestmark = pytest.mark.gpu
TOL = 1e-8
KERNEL = "sim_policy_vjp_kernel"


def _dev(x, env, dtype=None):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=dtype or env.dtype, device=env.device)


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def rounded(inp, dtype):
    """The inputs as the kernel sees them: rounded to the working dtype, as float64"""
    npdt = NP_DTYPE[dtype]
    r = lambda v: None if v is None else np.asarray(v).astype(npdt).astype(np.float64)
    out = dict(inp, W=[r(w) for w in inp["W"]], b=[r(b) for b in inp["b"]], noise=r(inp["noise"]), st=[r(v) for v in inp["st"]])
    out["refs"] = None if inp.get("refs") is None else {n: r(v) for n, v in inp["refs"].items()}
    return out


def forward(env, inp, activation, K, sub, tau, clip=hp.CLIP, control=None, noise=True, **kw):
    """One vmap_sim_ahead_policy call -> dict of its arguments and what it returned"""
    state = to_state(env, inp["st"], reference=inp["refs"] if control else None)
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], activation, device=env.device, dtype=env.dtype)
    nz = None
    if noise and K > 0:
        nz = env.new_actions_buffer(K)
        nz.copy_(_dev(inp["noise"][:, :K], env))
    obs, states, last, actions = env.vmap_sim_ahead_policy(state, policy, K, tau, tau * sub, noise=nz, clip=clip, **kw)
    return dict(env=env, state=state, policy=policy, noise=nz, obs=obs, states=states, last=last, actions=actions, K=K, sub=sub, tau=tau,
                clip=clip)


def explicit(run, group, **kw):
    """vmap_sim_ahead_policy_vjp on a forward run for one cotangent group -> dict of float64 numpy gradients named like the twin's"""
    env = run["env"]
    d = lambda v: None if v is None else _dev(v, env)
    dl = lambda vs: None if vs is None else [d(v) for v in vs]
    gs, gn, gp = env.vmap_sim_ahead_policy_vjp(
        run["policy"], run["obs"], run["states"], run["actions"], run["tau"], run["tau"] * run["sub"], clip=run["clip"],
        grad_obs=d(group.get("obs")), grad_states=dl(group.get("states")), grad_last_state=dl(group.get("last")),
        grad_actions=d(group.get("actions")) if run["K"] > 0 else None, **kw)
    assert env.last_policy_vjp_launch == KERNEL and _native.last_launch() == KERNEL
    torch.cuda.synchronize()
    B, K, A = env.batch_size, run["K"], env.action_dim
    assert tuple(gn.shape) == (B, K, A) and (gp is None or (gp.shape == run["policy"].params.shape and gp.dtype == env.dtype))
    return dict(state0=[_np(getattr(gs, n)) for n in env.STATE_FIELDS], noise=_np(gn), params=_np(gp), raw=(gs, gn, gp))


def compare(got, want, keep=None):
    """-> {name: relative distance} of every gradient (keep: environments compared, for the per-environment tensors)"""
    out = {f"state0[{j}]": rel_dist(g, w, keep) for j, (g, w) in enumerate(zip(got["state0"], want["state0"]))}
    if want["noise"] is not None and want["noise"].size:
        out["noise"] = rel_dist(got["noise"], want["noise"], keep)
    if got["params"] is not None:
        out["params"] = rel_dist(got["params"], want["params"])
    return out


def check(dist, bound, label):
    worst = max(dist.values())
    print(f"{label}: worst {worst:.3e} (bound {bound:.3e}) " + " ".join(f"{k}={v:.2e}" for k, v in dist.items()))
    assert worst <= bound, (label, dist)
    return worst


def masked(group, keep):
    """The cotangent group with zeros for the environments that are not kept: they then add nothing to any gradient on either side,
    the batch sum of grad_params included"""
    m = lambda v: None if v is None else np.asarray(v) * keep.reshape((-1,) + (1,) * (np.asarray(v).ndim - 1))
    return {k: ([m(x) for x in v] if isinstance(v, list) else m(v)) for k, v in group.items()}


# ---------------------------------------------------------------------------------------------------------------- 1
def _fp64_case(env_name, deadtime, solver, net, activation):
    spec, inp, twin, lv, out = hv.main_twin(env_name, deadtime, solver, net, activation)
    K, sub = hp.K_MAIN, hp.substeps_of(env_name)
    env, _, _, _ = make_env(env_name, hp.B_MAIN, torch.float64, solver, spec=spec)
    run = forward(env, inp, activation, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    groups = hv.cotangent_groups(np.random.default_rng(5), hp.B_MAIN, K * sub + 1, OW, S, K, A)
    keep = None
    if activation == "relu":  # an environment on a hidden kink has no derivative to compare
        keep = hv.keep_mask(twin, out, activation, margin=0.0, relu_margin=hv.RELU_MARGIN_FP64)
        print(f"{env_name} {net} relu: excluded {1 - float(np.mean(keep)):.4f}")
        assert 1 - float(np.mean(keep)) <= KINK_CAP
        groups = [masked(g, keep) for g in groups]
    want = hv.twin_grads(lv, out, groups)
    worst = 0.0
    for name, group, w in zip(hv.GROUP_NAMES, groups, want):
        worst = max(worst, check(compare(explicit(run, group), w, keep), TOL, f"{env_name} dead={deadtime} {solver} {net} {activation} [{name}]"))
    through = np.any(np.stack(want[3]["state0"]) != 0, axis=0)  # grad_actions alone: through the transposed network only
    reached = float(np.mean(through if keep is None else through[keep]))
    print(f"fp64 largest distance {env_name} dead={deadtime} {solver} {net} {activation}: {worst:.3e}; grad_actions alone reaches "
          f"state0 in {reached:.3f} of the environments")
    if net == "N1":  # (a ReLU network with few or many dead units, N3 / N2, passes nothing back in part of the batch)
        assert reached >= 0.9, reached


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_fp64_gradients_equal_the_twins(env_name, deadtime, solver, activation):
    _fp64_case(env_name, deadtime, solver, "N1", activation)


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("net", ["N2", "N0", "N3"])
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("pmsm", 1, "euler")])
def test_fp64_widest_deepest_and_smallest_networks(env_name, deadtime, solver, net, activation):
    _fp64_case(env_name, deadtime, solver, net, activation)


# ---------------------------------------------------------------------------------------------------------------- 2
FP32_CASES = [(e, d, s, "N1", a) for e, d in hp.CASES for s in hp.SOLVERS for a in ("tanh", "relu")]
FP32_CASES += [(e, d, s, n, "tanh") for e, d, s in (("pendulum", None, "tsit5"), ("pmsm", 1, "euler")) for n in ("N2", "N0")]


@pytest.mark.parametrize("env_name,deadtime,solver,net,activation", FP32_CASES)
def test_fp32_gradients_within_32_forward_floors(env_name, deadtime, solver, net, activation):
    """The floor: helpers_vjp.obs_floor of the fp32 policy launch (code this feature does not touch) against the twin on the same
    fp32-representable inputs, over the kept environments. Excluded: within KINK_MARGIN of a model kink or a clamp bound, or (ReLU)
    with a pre-activation below RELU_MARGIN; their cotangents are zero on both sides, so grad_params sums the kept ones only."""
    spec, inp64 = hp.main_case(env_name, deadtime, net)
    inp = rounded(inp64, torch.float32)
    K, sub = hp.K_MAIN, hp.substeps_of(env_name)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, activation, K, sub)
    keep = hv.keep_mask(twin, out, activation)
    excluded = 1.0 - float(np.mean(keep))
    env, _, _, _ = make_env(env_name, hp.B_MAIN, torch.float32, solver, spec=spec)
    run = forward(env, inp, activation, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    floor = obs_floor(_np(run["obs"]), out["obs"].detach().numpy(), env_name, keep)
    r32 = lambda v: np.asarray(v).astype(np.float32).astype(np.float64)
    worst = 0.0
    for name, group in zip(hv.GROUP_NAMES, hv.cotangent_groups(np.random.default_rng(5), hp.B_MAIN, K * sub + 1, OW, S, K, A)):
        if name in ("last_state", "obs"):
            continue  # the full group and the policy path alone
        group = masked({k: ([r32(x) for x in v] if isinstance(v, list) else r32(v)) for k, v in group.items()}, keep)
        want = hv.twin_grads(lv, out, [group])[0]
        dist = compare(explicit(run, group), want, keep)
        worst = max(worst, max(dist.values()))
        print(f"{env_name} dead={deadtime} {solver} {net} {activation} fp32 [{name}]: " + " ".join(f"{k}={v:.2e}" for k, v in dist.items()))
    print(f"{env_name} dead={deadtime} {solver} {net} {activation}: excluded {excluded:.4f}, forward floor {floor:.3e}, "
          f"worst {worst:.3e} = {worst / floor:.1f} floors")
    assert excluded <= KINK_CAP
    assert worst <= 32 * floor


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("acrobot", None, "rk4"), ("pmsm", 1, "euler"),
                                                     ("fluid_tank", None, "rk4")])
def test_zero_weights_are_the_open_loop_reverse_kernel_bit_for_bit(env_name, deadtime, solver):
    spec = case_spec(env_name, deadtime)
    B, K, sub = hp.B_MAIN, hp.K_MAIN, hp.substeps_of(env_name)
    inp = dict(hp.policy_inputs(env_name, spec, hp.NETS["N1"]))
    inp["W"] = [np.zeros_like(w) for w in inp["W"]]  # the biases stay as they are
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    group = hv.cotangent_groups(np.random.default_rng(13), B, K * sub + 1, OW, S, K, A)[0]
    group = dict(group, actions=None)
    for clip in (hp.CLIP, None):
        run = forward(env, inp, "tanh", K, sub, spec["tau"], clip=clip)
        got = explicit(run, group)
        again = explicit(run, group)
        keep = env.sim_ahead_semantics, env.launch_opts
        env.sim_ahead_semantics, env.launch_opts = "step", _native.launch_opts(envs_per_lane=1)
        try:
            ga, gs = env.vmap_sim_ahead_vjp(run["states"], run["actions"], spec["tau"], spec["tau"] * sub, _dev(group["obs"], env),
                                            [_dev(g, env) for g in group["states"]], [_dev(g, env) for g in group["last"]])
        finally:
            env.sim_ahead_semantics, env.launch_opts = keep
        torch.cuda.synchronize()
        same_state = all(torch.equal(getattr(gs, n), getattr(got["raw"][0], n)) for n in env.STATE_FIELDS)
        same_noise = torch.equal(ga, got["raw"][1])
        twice = all(torch.equal(getattr(again["raw"][0], n), getattr(got["raw"][0], n)) for n in env.STATE_FIELDS) and \
            torch.equal(again["raw"][1], got["raw"][1]) and torch.equal(again["raw"][2], got["raw"][2])
        print(f"{env_name} {solver} clip={clip}: grad_state0 == vmap_sim_ahead_vjp {same_state}; grad_noise == its action gradient "
              f"{same_noise}; two calls agree {twice}")
        assert same_state and twice
        if clip is None:
            assert same_noise
        assert float(np.abs(got["params"]).max()) > 0  # the parameters' own gradient is not zero at zero weights


FORM_CASES = [("pendulum", None, "rk4"), ("pmsm", 1, "euler")]


@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_recording_form_fills_the_grads_with_the_explicit_forms_bits(env_name, deadtime, solver):
    spec = case_spec(env_name, deadtime)
    B, K, sub = hp.B_MAIN, hp.K_MAIN, hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    plain = forward(env, inp, "tanh", K, sub, spec["tau"], differentiable=True)  # no input requires grad: the plain path
    assert plain["obs"].grad_fn is None and plain["actions"].grad_fn is None and env.last_policy_vjp_launch == ""
    group = hv.cotangent_groups(np.random.default_rng(14), B, K * sub + 1, OW, S, K, A)[0]
    want = explicit(plain, group)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], "tanh", device=env.device, dtype=env.dtype)
    policy.params.requires_grad_()
    nz = leaf(plain["noise"])
    st0 = [leaf(getattr(plain["state"].physical_state, n)) for n in env.STATE_FIELDS]
    s = env.State(env.PhysicalState(*st0), plain["state"].PRNGKey, plain["state"].additions, plain["state"].reference)
    obs, states, last, actions = env.vmap_sim_ahead_policy(s, policy, K, spec["tau"], spec["tau"] * sub, noise=nz, differentiable=True)
    assert all(t.grad_fn is not None for t in (obs, actions)) and torch.equal(obs, plain["obs"]) and torch.equal(actions, plain["actions"])
    d = lambda v: _dev(v, env)
    loss = (obs * d(group["obs"])).sum() + (actions * d(group["actions"])).sum()
    loss = loss + sum((getattr(states.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["states"]))
    loss = loss + sum((getattr(last.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["last"]))
    loss.backward()
    torch.cuda.synchronize()
    assert env.last_policy_vjp_launch == KERNEL
    gs, gn, gp = want["raw"]
    pairs = [("params", policy.params.grad, gp), ("noise", nz.grad, gn)] + [(n, l.grad, getattr(gs, n)) for n, l in zip(env.STATE_FIELDS, st0)]
    for name, a, b in pairs:
        print(f"{env_name} {name}: .grad == explicit form: {torch.equal(a, b)}")
        assert torch.equal(a, b), name


def test_a_reward_loss_reaches_a_tracked_torch_module():
    """vmap_generate_rew_trunc_term_ahead under env.differentiable composes, and from_torch(track=True) carries the gradient into the
    module: against the twin's gradient of the same loss"""
    from helpers_step_vjp import reward64

    env_name, deadtime, solver, control = "pmsm", 1, "rk4", ("i_d", "i_q")
    spec = case_spec(env_name, deadtime)
    B, K = hp.B_MAIN, hp.K_MAIN
    inp = hp.policy_inputs(env_name, spec, (6,), control=control)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, "tanh", K, 1, control=control)
    rew = sum(reward64(env_name, spec, control, [s[:, n] for s in out["states"]], inp["refs"]) for n in range(1, K + 1))
    gr = torch.autograd.grad(-rew.sum(), lv["W"] + lv["b"])
    want = hv.flat_params([g.numpy() for g in gr[:2]], [g.numpy() for g in gr[2:]])
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec, control_state=list(control))
    env.differentiable = True
    nn = torch.nn
    OW = env._obs_dim()
    module = nn.Sequential(nn.Linear(OW, 6), nn.Tanh(), nn.Linear(6, 2)).double().to(env.device)
    with torch.no_grad():
        for lin, W, b in zip((module[0], module[2]), inp["W"], inp["b"]):
            lin.weight.copy_(_dev(W, env))
            lin.bias.copy_(_dev(b, env))
    policy = excenvs.MLPPolicy.from_torch(module, track=True)
    state = to_state(env, inp["st"], reference=inp["refs"])
    obs, states, last, actions = env.vmap_sim_ahead_policy(state, policy, K, spec["tau"], spec["tau"], noise=_dev(inp["noise"], env),
                                                           differentiable=True)
    reward, _, _ = env.vmap_generate_rew_trunc_term_ahead(states, actions)
    (-reward.sum()).backward()
    torch.cuda.synchronize()
    got = hv.flat_params([_np(module[0].weight.grad), _np(module[2].weight.grad)], [_np(module[0].bias.grad), _np(module[2].bias.grad)])
    check(dict(params=rel_dist(got, want)), TOL, "pmsm reward loss into the module's .grad")


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("solver", ["euler", "tsit5"])
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_gradients_equal_the_chain_of_differentiable_steps(env_name, deadtime, solver, activation):
    """Each side holds 1e-8 to the twin (test 1 here, tests/test_gpu_step_vjp.py there): 2e-8 between them."""
    B, K = hp.B_MAIN, 4
    spec = case_spec(env_name, deadtime)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"], B, K)
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    run = forward(env, inp, activation, K, 1, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    group = hv.cotangent_groups(np.random.default_rng(6), B, K + 1, OW, S, K, A)[0]
    keep = None
    if activation == "relu":
        twin, _, out = hv.twin_run(env_name, spec, solver, inp, activation, K, 1)
        keep = hv.keep_mask(twin, out, activation, margin=0.0, relu_margin=hv.RELU_MARGIN_FP64)
        group = masked(group, keep)
    got = explicit(run, group)
    # the parent's route: K differentiable vmap_step calls, the network in torch
    env.differentiable = True
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    p, nz = leaf(run["policy"].params), leaf(run["noise"])
    st0 = [leaf(getattr(run["state"].physical_state, n)) for n in env.STATE_FIELDS]
    s = env.State(env.PhysicalState(*st0), run["state"].PRNGKey, run["state"].additions, run["state"].reference)
    ob = Twin(env_name, spec, solver, "step").observe(st0)  # row 0's observation with a graph (the package's own is a kernel without one)
    d = lambda v: _dev(v, env)
    lo, hi = hp.CLIP
    loss = (ob * d(group["obs"][:, 0])).sum() + sum((l * d(g[:, 0])).sum() for l, g in zip(st0, group["states"]))
    acts = []
    for k in range(K):
        raw = nz[:, k] + run["policy"].torch_forward(ob, p)
        a = torch.where((raw > lo) & (raw < hi), raw, raw.detach().clamp(lo, hi))
        acts.append(a)
        ob, s = env.vmap_step(s, a)
        loss = loss + (ob * d(group["obs"][:, k + 1])).sum() + (a * d(group["actions"][:, k])).sum()
        loss = loss + sum((getattr(s.physical_state, n) * d(g[:, k + 1])).sum() for n, g in zip(env.STATE_FIELDS, group["states"]))
    loss = loss + sum((getattr(s.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["last"]))
    gr = torch.autograd.grad(loss, st0 + [nz, p])
    torch.cuda.synchronize()
    env.differentiable = False
    da = float((torch.stack(acts, dim=1).detach() - run["actions"]).abs().max())
    print(f"{env_name} dead={deadtime} {solver} {activation}: forward actions of the chain within {da:.3e}")
    want = dict(state0=[_np(g) for g in gr[:S]], noise=_np(gr[S]), params=_np(gr[S + 1]))
    check(compare(got, want, keep), 2e-8, f"{env_name} dead={deadtime} {solver} {activation} vs the chain of steps")


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("env_name,deadtime", [("pendulum", None), ("pmsm", 0)])
def test_directional_finite_difference_through_the_forward_launch(env_name, deadtime):
    """Per environment: <grad_state0, d_state> + <grad_noise, d_noise> + <grad_noise, J_params mlp(obs) d_params> against
    (L(+h) - L(-h)) / 2h of forward launches along the direction (d_state, d_noise, d_params); h and the bound are those of
    tests/test_gpu_feedback_vjp.py's directional test (1e-5, 1e-6 of the largest derivative). The batch sum of the third term must
    be <grad_params, d_params>. Environments inside KINK_MARGIN of a kink or clamp bound are excluded."""
    solver, h, activation = "rk4", 1e-5, "tanh"
    spec = case_spec(env_name, deadtime)
    B, K, sub = hp.B_MAIN, hp.K_MAIN, hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    twin, _, out = hv.twin_run(env_name, spec, solver, inp, activation, K, sub)
    keep = hv.keep_mask(twin, out, activation)
    rng = np.random.default_rng(15)
    d_st = [rng.normal(size=B) * 0.01 * float(np.max(np.abs(v))) for v in inp["st"]]
    d_nz = rng.normal(size=inp["noise"].shape)
    d_W, d_b = [rng.normal(size=w.shape) * 0.1 for w in inp["W"]], [rng.normal(size=b.shape) * 0.1 for b in inp["b"]]
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    OW = env._obs_dim()
    w = rng.normal(size=(B, K * sub + 1, OW))

    def obs_rows(sign):
        moved = dict(inp, st=[v + sign * h * d for v, d in zip(inp["st"], d_st)], noise=inp["noise"] + sign * h * d_nz,
                     W=[v + sign * h * d for v, d in zip(inp["W"], d_W)], b=[v + sign * h * d for v, d in zip(inp["b"], d_b)])
        return _np(forward(env, moved, activation, K, sub, spec["tau"])["obs"])

    run = forward(env, inp, activation, K, sub, spec["tau"])
    got = explicit(run, dict(obs=w))
    dp = _dev(hv.flat_params(d_W, d_b), env)
    rows_k = run["obs"][:, 0:K * sub:sub, :]
    _, jv = torch.autograd.functional.jvp(lambda q: run["policy"].torch_forward(rows_k, q), run["policy"].params, dp)
    par = (got["noise"] * _np(jv)).sum(axis=(1, 2))
    dd = sum(g * d for g, d in zip(got["state0"], d_st)) + (got["noise"] * d_nz).sum(axis=(1, 2)) + par
    fd = (w * (obs_rows(+1) - obs_rows(-1))).sum(axis=(1, 2)) / (2 * h)
    scale = float(np.max(np.abs(fd[keep])))
    err = float(np.max(np.abs(dd - fd)[keep])) / scale
    total = abs(float((got["params"] * _np(dp)).sum()) - float(par.sum())) / float(np.abs(par).sum())
    print(f"{env_name} dead={deadtime}: directional derivative rel err {err:.3e} (scale {scale:.3e}), excluded {1 - float(np.mean(keep)):.4f}; "
          f"<grad_params, d> against the batch sum {total:.3e}; parameter share {float(np.abs(par[keep]).max()) / scale:.3f}")
    assert 1 - float(np.mean(keep)) <= KINK_CAP
    assert err <= 1e-6 and total <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_episode_mask_against_the_twin_with_the_same_mask(env_name, deadtime, solver):
    """Case E2 of helpers_episodes (a budget of two steps: three resets per environment in nine rows). The twin takes the reset rows
    from the launch's own state trajectory as constants (torch.where on the returned mask)."""
    import helpers_episodes as he

    spec = case_spec(env_name, deadtime)
    inp = he.episode_inputs(env_name, spec, "E2")
    control, B, K, tau = inp["control"], he.B, he.K, spec["tau"]
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec, control_state=list(control))
    state = to_state(env, inp["st"], reference=inp["refs"])
    rows = [to_state(env, r, reference=inp["refs"]) for r in inp["reset"]]
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], "tanh", device=env.device, dtype=env.dtype)
    ro = env.vmap_rollout_episodes(state, policy, K, tau, rows, noise=_dev(inp["noise"], env), max_episode_steps=inp["max_episode_steps"],
                                   episode_steps=_dev(inp["steps_in"], env, torch.int32))
    reset = ro.reset.cpu().numpy()
    n_resets = ro.n_resets.cpu().numpy()
    print(f"{env_name}: resets per environment {n_resets.min()} .. {n_resets.max()}, share of reset steps {reset.mean():.3f}")
    assert n_resets.min() >= 3
    traj = [_np(getattr(ro.states.physical_state, n)) for n in env.STATE_FIELDS]
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, "tanh", K, 1, control=control, reset=reset, reset_rows=traj)
    fwd = rel_dist(_np(ro.observations), out["obs"].detach().numpy())
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    groups = hv.cotangent_groups(np.random.default_rng(16), B, K + 1, OW, S, K, A)
    want = hv.twin_grads(lv, out, groups)
    run = dict(env=env, policy=policy, obs=ro.observations, states=ro.states, actions=ro.actions, K=K, sub=1, tau=tau, clip=hp.CLIP)
    print(f"{env_name}: forward rows of the twin within {fwd:.3e}")
    for name, group, w in zip(hv.GROUP_NAMES, groups, want):
        check(compare(explicit(run, group, reset=ro.reset), w), TOL, f"{env_name} episodes [{name}]")
    # the mask matters: without it the same call gives other gradients
    other = explicit(run, groups[0])
    assert max(compare(other, want[0]).values()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- 7
def _form(env_name, deadtime, solver, B, K, net="N1", activation="tanh", control=None, clip=hp.CLIP, noise=True, seed=hp.SEED, groups=(0,),
          **kw):
    """One form in fp64: the explicit form's gradients and the twin's for the chosen cotangent groups"""
    spec = case_spec(env_name, deadtime)
    sub = hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS[net], B, K, control=control, seed=seed)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, activation, K, sub, clip=clip, control=control, noise=noise)
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec, control_state=list(control) if control else None)
    run = forward(env, inp, activation, K, sub, spec["tau"], clip=clip, control=control, noise=noise)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    all_groups = hv.cotangent_groups(np.random.default_rng(11), B, K * sub + 1, OW, S, K, A)
    chosen = [all_groups[j] for j in groups]
    return [explicit(run, g, **kw) for g in chosen], hv.twin_grads(lv, out, chosen), run, (lv, out), chosen


@pytest.mark.parametrize("what", ["no_noise", "no_clip"])
@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_without_noise_and_without_clamp(env_name, deadtime, solver, what):
    got, want, run, _, _ = _form(env_name, deadtime, solver, hp.B_MAIN, hp.K_MAIN, clip=None if what == "no_clip" else hp.CLIP,
                                 noise=what != "no_noise", groups=(0, 3))
    for g, w in zip(got, want):
        assert g["noise"] is not None  # the gradient with respect to the pre-clamp output is returned all the same
        check(compare(g, w), TOL, f"{env_name} {what}")


@pytest.mark.parametrize("env_name,deadtime,control", [("pendulum", None, ("theta", "omega")), ("pmsm", 0, ("i_d", "i_q"))])
def test_two_control_columns_their_weights_get_gradients(env_name, deadtime, control):
    got, want, run, inp, groups = _form(env_name, deadtime, "rk4", hp.B_MAIN, hp.K_MAIN, control=control, groups=(0, 3))
    for g, w in zip(got, want):
        check(compare(g, w), TOL, f"{env_name} control {control}")
    O, d1 = hp.obs_width(env_name), hp.NETS["N1"][0]
    W1 = got[0]["params"][:d1 * (O + 2)].reshape(d1, O + 2)
    print(f"{env_name}: largest gradient of a first-layer weight on a reference column {float(np.abs(W1[:, O:]).max()):.3e}")
    assert float(np.abs(W1[:, O:]).max()) > 0
    # the control columns of grad_obs are ignored: another cotangent there, the same bits
    moved = dict(groups[0], obs=groups[0]["obs"].copy())
    moved["obs"][:, :, O:] += 3.0
    again = explicit(run, moved)
    assert all(torch.equal(getattr(again["raw"][0], n), getattr(got[0]["raw"][0], n)) for n in run["env"].STATE_FIELDS)
    assert torch.equal(again["raw"][1], got[0]["raw"][1]) and torch.equal(again["raw"][2], got[0]["raw"][2])


@pytest.mark.parametrize("B,K", [(hp.B_MAIN, 1), (hp.B_MAIN, 0), (1, hp.K_MAIN), (64, hp.K_MAIN), (65, hp.K_MAIN), (1, 0)])
@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_single_rows_no_rows_and_batch_edges(env_name, deadtime, solver, B, K):
    got, want, run, _, _ = _form(env_name, deadtime, solver, B, K, seed=hp.SEED + 10 * B + K, groups=(0, 3) if K else (0,))
    for g, w in zip(got, want):
        assert g["noise"].shape == (B, K, run["env"].action_dim)
        check(compare(g, w), TOL, f"{env_name} B={B} K={K}")
    if K == 0:
        assert float(np.abs(got[0]["params"]).max()) == 0.0


@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_absent_cotangent_groups_and_the_launch_alone(env_name, deadtime, solver):
    got, want, run, (lv, out), groups = _form(env_name, deadtime, solver, hp.B_MAIN, hp.K_MAIN, net="N2", groups=(0, 1, 2, 3))
    for name, g, w in zip(hv.GROUP_NAMES, got, want):
        check(compare(g, w), TOL, f"{env_name} N2 [{name}]")
    S = run["env"].physical_state_dim
    some = dict(states=[groups[0]["states"][0]] + [None] * (S - 1), last=[None] * (S - 1) + [groups[0]["last"][-1]])
    env = run["env"]
    check(compare(explicit(run, some), hv.twin_grads(lv, out, [some])[0]), TOL, f"{env_name} single leaves")
    alone = explicit(run, groups[0], param_grads=False)
    assert alone["params"] is None and torch.equal(alone["raw"][1], got[0]["raw"][1])
    assert all(torch.equal(getattr(alone["raw"][0], n), getattr(got[0]["raw"][0], n)) for n in env.STATE_FIELDS)
