"""The policy's parameter gradient on the matrix cores, on the GPU (excenv_policy_param_grad: policy_param_grad_kernel and
policy_param_grad_reduce_kernel; `vmap_policy_param_grads`, `vmap_sim_ahead_policy_vjp(param_grads="fused")`,
`env.policy_param_grads = "fused"`):
1. the entry alone on random arrays against the float64 restatement (helpers_policy_param_grad), fp64, 1e-8 of the largest magnitude;
2. a derived fp32 bound without a hidden layer, per entry;
3. the flush path (one workgroup over more than EXCENV_PARAM_GRAD_CHAIN samples), the groupings among each other, equal bits twice;
4. through the rollout against the float64 torch twin, the torch route's distance beside each;
5. forms: control columns, the episode mask, K = 0, the recording form and a tracked module.
Every case prints its figures."""
import functools

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_policy as hp
import helpers_policy_param_grad as hg
import helpers_policy_vjp as hv
import test_gpu_policy_vjp as base
from exciting_environments_amd import _native
from helpers import make_env, to_state
from helpers_vjp import KINK_CAP, case_spec, obs_floor, rel_dist

pytestmark = pytest.mark.gpu
TOL = 1e-8
KERNEL = "policy_param_grad_kernel"
U32 = 2.0 ** -24
_dev, _np = base._dev, base._np


@functools.lru_cache(maxsize=None)
def _env(B, dtype):
    return make_env("pendulum", B, dtype)[0]


def fused_entry(case, activation, dtype=torch.float64, max_groups=0, sub=3):
    """vmap_policy_param_grads on the arrays of a helpers_policy_param_grad case -> the flat gradient (device tensor)"""
    B = case["obs"].shape[0]
    env = _env(B, dtype)
    policy = excenvs.MLPPolicy(case["W"], case["b"], activation, device=env.device, dtype=env.dtype)
    got = env.vmap_policy_param_grads(policy, _dev(case["obs"], env), _dev(case["graw"], env), env.tau, env.tau * sub, max_groups=max_groups)
    assert _native.last_launch() == KERNEL
    torch.cuda.synchronize()
    assert got.shape == policy.params.shape and got.dtype == dtype
    return got


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("net,activation,OW,A,B,K", hg.ENTRY_CASES)
def test_entry_alone_equals_the_float64_restatement(net, activation, OW, A, B, K):
    case = hg.entry_case(net, activation, OW, A, B, K)
    want = hg.restatement(case["W"], case["b"], activation, case["rows"], case["g"])
    got = _np(fused_entry(case, activation))
    d = rel_dist(got, want)
    print(f"{net} {activation} OW={OW} A={A} B={B} K={K}: largest distance {d:.3e} of {float(np.abs(want).max()):.3e}"
          + (f", smallest |pre-activation| {case['relu_min']:.2e}" if activation == "relu" else ""))
    assert d <= TOL


# ---------------------------------------------------------------------------------------------------------------- 2
def _n0_exact(case):
    """Without a hidden layer dW[q][i] = sum g x and db[q] = sum g: the exact sums in float64 and the sums of magnitudes, flat"""
    x1 = np.concatenate([case["rows"], np.ones((len(case["rows"]), 1))], axis=1)
    A, OW = case["g"].shape[1], case["rows"].shape[1]
    full = np.einsum("nq,ni->qi", case["g"], x1)
    mag = np.einsum("nq,ni->qi", np.abs(case["g"]), np.abs(x1))
    flat = lambda m: np.concatenate([m[:, :OW].reshape(-1), m[:, OW]])
    return flat(full), flat(mag), A * (OW + 1)


@pytest.mark.parametrize("K", [hp.K_MAIN, 40])
def test_fp32_without_a_hidden_layer_within_the_summation_bound(K):
    """|fused - exact64| <= (n + G + 2) 2^-24 sum |g x| per entry, n = B K: the gamma_n bound of any summation order of the products
    the kernel reads exactly, one rounding per partial and the store"""
    B = hp.B_MAIN
    case = hg.random_case((8, 2), "tanh", B, K, 3, 1, "float32")
    want, mag, P = _n0_exact(case)
    got = _np(fused_entry(case, "tanh", torch.float32))
    n, G = B * K, hg.groups(B, K)
    bound = (n + G + 2) * U32 * mag
    ratio = float(np.max(np.abs(got - want) / bound))
    print(f"N0 fp32 B={B} K={K}: n={n} G={G}; largest |fused - exact| / bound {ratio:.3e}; largest error {float(np.abs(got - want).max()):.3e}")
    assert got.shape == (P,) and np.all(np.abs(got - want) <= bound)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_flush_path_and_groupings():
    B, K = hp.B_MAIN, 40
    assert hg.tiles(B, K) == 240 and B * K == 13040 > _native.PARAM_GRAD_CHAIN
    assert hg.tile_ranges(B, K, 1) == [(0, 240)]
    # fp64, N1, both activations: every grouping within the bound, the groupings among each other, two calls the same bits
    for activation in hp.ACTIVATIONS:
        case = hg.entry_case("N1", activation, 8, 2, B, K)
        want = hg.restatement(case["W"], case["b"], activation, case["rows"], case["g"])
        got = {mg: fused_entry(case, activation, max_groups=mg) for mg in (1, 3, 0)}
        for mg, g in got.items():
            d = rel_dist(_np(g), want)
            again = fused_entry(case, activation, max_groups=mg)
            print(f"N1 {activation} fp64 max_groups={mg}: distance {d:.3e}; two calls equal bits {torch.equal(g, again)}")
            assert d <= TOL and torch.equal(g, again)
        pair = max(rel_dist(_np(got[a]), _np(got[b])) for a, b in ((1, 3), (1, 0), (3, 0)))
        print(f"N1 {activation} fp64: groupings among each other {pair:.3e}")
        assert pair <= TOL
    # fp32 without a hidden layer: the derived bound with one workgroup
    case = hg.random_case((8, 2), "tanh", B, K, 3, 1, "float32")
    want, mag, _ = _n0_exact(case)
    for mg in (1, 3):
        got32 = fused_entry(case, "tanh", torch.float32, max_groups=mg)
        bound = (B * K + hg.groups(B, K, mg) + 2) * U32 * mag
        ratio = float(np.max(np.abs(_np(got32) - want) / bound))
        print(f"N0 fp32 max_groups={mg}: largest |fused - exact| / bound {ratio:.3e}")
        assert np.all(np.abs(_np(got32) - want) <= bound) and torch.equal(got32, fused_entry(case, "tanh", torch.float32, max_groups=mg))
    # fp32 N1: a grouping changes the order of the sums only (every sample's recomputation is the same statements on the same
    # values, so its terms have the same bits), and each grouping lies within (n + G + 2) 2^-24 sum |term| of the exact sum of those
    # terms. Two groupings therefore differ per entry by at most the sum of their two bounds; the magnitudes come from the float64
    # backpropagation (helpers_policy_param_grad.term_magnitudes) with 1 % for the terms' own fp32 error.
    case = hg.entry_case("N1", "tanh", 8, 2, B, K, "float32")
    want = hg.restatement(case["W"], case["b"], "tanh", case["rows"], case["g"])
    mag = 1.01 * hg.term_magnitudes(case["W"], case["b"], "tanh", case["rows"], case["g"])
    one, auto = (fused_entry(case, "tanh", torch.float32, max_groups=mg) for mg in (1, 0))
    bound = (2 * B * K + 1 + hg.groups(B, K) + 4) * U32 * mag
    ratio = float(np.max(np.abs(_np(one) - _np(auto)) / bound))
    twice = torch.equal(one, fused_entry(case, "tanh", torch.float32, max_groups=1))
    print(f"N1 tanh fp32: max_groups=1 within {rel_dist(_np(one), want):.3e} of the restatement, auto within {rel_dist(_np(auto), want):.3e}; "
          f"|one - auto| / bound {ratio:.3e}; two calls equal bits {twice}")
    assert twice and np.all(np.abs(_np(one) - _np(auto)) <= bound)


# ---------------------------------------------------------------------------------------------------------------- 4
def explicit(run, group, param_grads, **kw):
    """vmap_sim_ahead_policy_vjp on a forward run for one cotangent group -> dict of float64 numpy gradients named like the twin's"""
    env = run["env"]
    d = lambda v: None if v is None else _dev(v, env)
    dl = lambda vs: None if vs is None else [d(v) for v in vs]
    gs, gn, gp = env.vmap_sim_ahead_policy_vjp(
        run["policy"], run["obs"], run["states"], run["actions"], run["tau"], run["tau"] * run["sub"], clip=run["clip"],
        grad_obs=d(group.get("obs")), grad_states=dl(group.get("states")), grad_last_state=dl(group.get("last")),
        grad_actions=d(group.get("actions")) if run["K"] > 0 else None, param_grads=param_grads, **kw)
    assert env.last_policy_vjp_launch == "sim_policy_vjp_kernel"
    if param_grads == "fused" and env.batch_size > 0:
        assert _native.last_launch() == KERNEL
    torch.cuda.synchronize()
    return dict(state0=[_np(getattr(gs, n)) for n in env.STATE_FIELDS], noise=_np(gn), params=_np(gp), raw=(gs, gn, gp))


def same_bits(a, b, env):
    return all(torch.equal(getattr(a["raw"][0], n), getattr(b["raw"][0], n)) for n in env.STATE_FIELDS) and torch.equal(a["raw"][1], b["raw"][1])


def _rollout_case(env_name, deadtime, solver, net, activation, label):
    spec, inp, twin, lv, out = hv.main_twin(env_name, deadtime, solver, net, activation)
    K, sub = hp.K_MAIN, hp.substeps_of(env_name)
    env, _, _, _ = make_env(env_name, hp.B_MAIN, torch.float64, solver, spec=spec)
    run = base.forward(env, inp, activation, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    groups = hv.cotangent_groups(np.random.default_rng(5), hp.B_MAIN, K * sub + 1, OW, S, K, A)
    groups = [groups[0], groups[3]]  # all; grad_actions alone
    if activation == "relu":
        keep = hv.keep_mask(twin, out, activation, margin=0.0, relu_margin=hv.RELU_MARGIN_FP64)
        assert 1 - float(np.mean(keep)) <= KINK_CAP
        groups = [base.masked(g, keep) for g in groups]
    want = hv.twin_grads(lv, out, groups)
    for name, group, w in zip(("all", "actions"), groups, want):
        got, torch_route, alone = explicit(run, group, "fused"), explicit(run, group, "torch"), explicit(run, group, False)
        d, dt = rel_dist(got["params"], w["params"]), rel_dist(torch_route["params"], w["params"])
        print(f"{label} [{name}]: grad_params fused {d:.3e}, torch route {dt:.3e} (bound {TOL:.0e})")
        assert d <= TOL
        assert alone["params"] is None and same_bits(got, alone, env)


@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_fp64_through_the_rollout_equals_the_twin(env_name, deadtime):
    _rollout_case(env_name, deadtime, "euler", "N1", "tanh", f"{env_name} dead={deadtime} euler N1 tanh")


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("net", ["N2", "N0", "N3"])
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("pmsm", 1, "euler")])
def test_fp64_through_the_rollout_other_networks(env_name, deadtime, solver, net, activation):
    _rollout_case(env_name, deadtime, solver, net, activation, f"{env_name} dead={deadtime} {solver} {net} {activation}")


@pytest.mark.parametrize("net,activation", [("N1", "tanh"), ("N2", "tanh"), ("N1", "relu")])
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("pmsm", 1, "euler")])
def test_fp32_through_the_rollout_within_32_forward_floors(env_name, deadtime, solver, net, activation):
    """The rule of tests/test_gpu_policy_vjp.py: helpers_vjp.obs_floor of the fp32 policy launch against the twin on the same
    fp32-representable inputs; environments inside the margins have zero cotangents on both sides"""
    spec, inp64 = hp.main_case(env_name, deadtime, net)
    inp = base.rounded(inp64, torch.float32)
    K, sub = hp.K_MAIN, hp.substeps_of(env_name)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, activation, K, sub)
    keep = hv.keep_mask(twin, out, activation)
    excluded = 1.0 - float(np.mean(keep))
    env, _, _, _ = make_env(env_name, hp.B_MAIN, torch.float32, solver, spec=spec)
    run = base.forward(env, inp, activation, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    floor = obs_floor(_np(run["obs"]), out["obs"].detach().numpy(), env_name, keep)
    r32 = lambda v: np.asarray(v).astype(np.float32).astype(np.float64)
    groups = hv.cotangent_groups(np.random.default_rng(5), hp.B_MAIN, K * sub + 1, OW, S, K, A)
    assert excluded <= KINK_CAP
    for name, group in (("all", groups[0]), ("actions", groups[3])):
        group = base.masked({k: ([r32(x) for x in v] if isinstance(v, list) else r32(v)) for k, v in group.items()}, keep)
        want = hv.twin_grads(lv, out, [group])[0]
        got, torch_route, alone = explicit(run, group, "fused"), explicit(run, group, "torch"), explicit(run, group, False)
        d, dt = rel_dist(got["params"], want["params"]), rel_dist(torch_route["params"], want["params"])
        print(f"{env_name} dead={deadtime} {solver} {net} {activation} fp32 [{name}]: excluded {excluded:.4f}, forward floor {floor:.3e}; "
              f"grad_params fused {d:.3e} = {d / floor:.1f} floors, torch route {dt:.3e} = {dt / floor:.1f} floors")
        assert d <= 32 * floor
        assert same_bits(got, alone, env)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_two_control_columns_their_weights_get_gradients():
    env_name, control = "pendulum", ("theta", "omega")
    got, want, run, _, groups = base._form(env_name, None, "rk4", hp.B_MAIN, hp.K_MAIN, control=control, groups=(0, 3), param_grads=False)
    O, d1 = hp.obs_width(env_name), hp.NETS["N1"][0]
    for group, w in zip(groups, want):
        g = explicit(run, group, "fused")
        d = rel_dist(g["params"], w["params"])
        W1 = g["params"][:d1 * (O + 2)].reshape(d1, O + 2)
        W1w = w["params"][:d1 * (O + 2)].reshape(d1, O + 2)
        dref = rel_dist(W1[:, O:], W1w[:, O:])
        print(f"{env_name} control {control}: grad_params {d:.3e}; weights on reference columns {dref:.3e} of {float(np.abs(W1w[:, O:]).max()):.3e}")
        assert d <= TOL and dref <= TOL and float(np.abs(W1[:, O:]).max()) > 0


def test_episode_mask_is_carried_by_grad_raw():
    import helpers_episodes as he

    env_name, solver = "pendulum", "rk4"
    spec = case_spec(env_name, None)
    inp = he.episode_inputs(env_name, spec, "E2")
    control, B, K, tau = inp["control"], he.B, he.K, spec["tau"]
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec, control_state=list(control))
    state = to_state(env, inp["st"], reference=inp["refs"])
    rows = [to_state(env, r, reference=inp["refs"]) for r in inp["reset"]]
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], "tanh", device=env.device, dtype=env.dtype)
    ro = env.vmap_rollout_episodes(state, policy, K, tau, rows, noise=_dev(inp["noise"], env), max_episode_steps=inp["max_episode_steps"],
                                   episode_steps=_dev(inp["steps_in"], env, torch.int32))
    reset = ro.reset.cpu().numpy()
    traj = [_np(getattr(ro.states.physical_state, n)) for n in env.STATE_FIELDS]
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, "tanh", K, 1, control=control, reset=reset, reset_rows=traj)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    groups = hv.cotangent_groups(np.random.default_rng(16), B, K + 1, OW, S, K, A)
    groups = [groups[0], groups[3]]
    want = hv.twin_grads(lv, out, groups)
    run = dict(env=env, policy=policy, obs=ro.observations, states=ro.states, actions=ro.actions, K=K, sub=1, tau=tau, clip=hp.CLIP)
    for name, group, w in zip(("all", "actions"), groups, want):
        g = explicit(run, group, "fused", reset=ro.reset)
        d = rel_dist(g["params"], w["params"])
        print(f"{env_name} episodes E2 [{name}]: grad_params fused {d:.3e}, share of reset steps {reset.mean():.3f}")
        assert d <= TOL
    # grad_raw on its own through the entry: the same bits as the fused route
    g = explicit(run, groups[0], "fused", reset=ro.reset)
    alone = env.vmap_policy_param_grads(policy, ro.observations, g["raw"][1], tau, tau)
    assert torch.equal(alone, g["raw"][2])


def test_no_action_rows_give_zeros():
    got, want, run, _, groups = base._form("pendulum", None, "rk4", hp.B_MAIN, 0, groups=(0,), param_grads=False)
    g = explicit(run, groups[0], "fused")
    assert g["params"].shape == want[0]["params"].shape and float(np.abs(g["params"]).max()) == 0.0
    env = run["env"]
    direct = env.vmap_policy_param_grads(run["policy"], run["obs"], torch.full((hp.B_MAIN, 0, 1), float("nan"), dtype=env.dtype, device=env.device),
                                         run["tau"], run["tau"] * run["sub"])
    torch.cuda.synchronize()
    assert _native.last_launch() == KERNEL and float(direct.abs().max()) == 0.0


@pytest.mark.parametrize("route", ["fused", "torch"])
def test_recording_form_follows_the_environments_setting(route):
    """env.policy_param_grads = "fused" fills policy.params.grad, and a tracked module's .grad, with the explicit fused form's bits;
    with the default setting the recording form still gives the torch route's bits"""
    env_name, solver = "pendulum", "rk4"
    spec = case_spec(env_name, None)
    B, K, sub = hp.B_MAIN, hp.K_MAIN, hp.substeps_of(env_name)
    inp = hp.policy_inputs(env_name, spec, hp.NETS["N1"])
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    assert env.policy_param_grads == "torch"
    if route == "fused":
        env.policy_param_grads = "fused"
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    plain = base.forward(env, inp, "tanh", K, sub, spec["tau"])
    group = hv.cotangent_groups(np.random.default_rng(14), B, K * sub + 1, OW, S, K, A)[0]
    want = explicit(plain, group, route)
    other = explicit(plain, group, "torch" if route == "fused" else "fused")
    d = lambda v: _dev(v, env)

    def loss_of(obs, states, last, actions):
        loss = (obs * d(group["obs"])).sum() + (actions * d(group["actions"])).sum()
        loss = loss + sum((getattr(states.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["states"]))
        return loss + sum((getattr(last.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["last"]))

    policy = excenvs.MLPPolicy(inp["W"], inp["b"], "tanh", device=env.device, dtype=env.dtype)
    policy.params.requires_grad_()
    loss_of(*env.vmap_sim_ahead_policy(plain["state"], policy, K, spec["tau"], spec["tau"] * sub, noise=plain["noise"], differentiable=True)).backward()
    torch.cuda.synchronize()
    differ = not torch.equal(want["raw"][2], other["raw"][2])
    print(f"{route}: .grad == explicit {route} form {torch.equal(policy.params.grad, want['raw'][2])}; the two routes differ in bits: {differ}")
    assert torch.equal(policy.params.grad, want["raw"][2])
    # a tracked module
    nn = torch.nn
    d1, d2 = hp.NETS["N1"]
    module = nn.Sequential(nn.Linear(OW, d1), nn.Tanh(), nn.Linear(d1, d2), nn.Tanh(), nn.Linear(d2, A)).to(device=env.device, dtype=env.dtype)
    with torch.no_grad():
        for lin, W, b in zip([m for m in module if isinstance(m, nn.Linear)], inp["W"], inp["b"]):
            lin.weight.copy_(d(W))
            lin.bias.copy_(d(b))
    tracked = excenvs.MLPPolicy.from_torch(module, track=True)
    loss_of(*env.vmap_sim_ahead_policy(plain["state"], tracked, K, spec["tau"], spec["tau"] * sub, noise=plain["noise"], differentiable=True)).backward()
    torch.cuda.synchronize()
    flat = torch.cat([t.grad.reshape(-1) for lin in module if isinstance(lin, nn.Linear) for t in (lin.weight, lin.bias)])
    assert torch.equal(flat, want["raw"][2])
