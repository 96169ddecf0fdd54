"""Host side of the policy rollout's reverse mode (no GPU):
- the header and its `_native` mirror; excenv_sim_policy_vjp refuses by code and whole message, before any launch, what it does not
  do; the empty batch; the bytes function is the formula of include/excenv.h / DESIGN.md §4.15;
- the 36 built sim_policy_vjp_kernel instantiations use no scratch memory and no static LDS, and the LDS formula of a launch;
- the Python methods refuse by name what they do not do, and the default keyword of vmap_sim_ahead_policy still refuses;
- MLPPolicy.torch_forward is helpers_policy.mlp_np; MLPPolicy.from_torch(track=True) reaches a module's .grad;
- the float64 torch twin of tests/helpers_policy_vjp.py gives the forward of helpers_policy.oracle_policy_loop, and its inputs meet
  the conditions the GPU tests rely on (the excluded share; grad_actions alone reaches the initial state through the network)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import helpers_policy as hp
import helpers_policy_vjp as hv
from exciting_environments_amd import EnvironmentRegistry, MLPPolicy, _native
from helpers import ANGLE_OBS
from helpers_budget import budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
MODELS = ["Pendulum", "MassSpringDamper", "CartPole", "Acrobot", "FluidTank", "Pmsm"]
FN = "excenv_sim_policy_vjp"


# ---- header, mirror, kernels ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_sim_policy_vjp\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_sim_policy_vjp_bytes\s*\(", hdr)
    assert re.search(r"\}\s*excenv_policy_vjp_t\s*;", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # additions: a binder probes for the symbols
    lib = ctypes.CDLL(_native.library_path())
    assert all(hasattr(lib, n) for n in (FN, FN + "_bytes"))
    assert len(_native.PROTOTYPES[FN][1]) == 13 and len(_native.PROTOTYPES[FN + "_bytes"][1]) == 8
    assert _native.STRUCTS[_native.PolicyVjp] == "excenv_policy_vjp_t"
    names = [n for n, _ in _native.PolicyVjp._fields_]
    assert names == ["policy", "obs_traj", "state_traj", "actions", "reset", "grad_obs", "grad_states", "grad_last_state", "grad_actions",
                     "grad_state0", "grad_raw"]
    assert _native.PolicyVjp.policy.size == ctypes.sizeof(_native.Policy) and _native.PolicyVjp.policy.offset == 0


def test_kernels_exist_without_scratch_and_the_lds_formula():
    """tools/loop_code_size.py on the built library: the 36 instantiations (six models x three solvers x two element types) are all
    there, none for the saturated PMSM, no scratch memory, no static LDS (the launch sizes it), at most the 512 registers of one wave
    per SIMD. The dynamic LDS is every hidden layer at once, 64 lanes wide."""
    res, spans = budget("sim_policy_vjp_kernel")
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"sim_policy_vjp_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]} loop/kernel bytes {spans[hit[0]]}")
    assert len(res) == 36, len(res)
    over = {k: v for k, v in res.items() if v["scratch"] != 0 or v["lds"] != 0 or v["vgpr"] > 512}
    assert not over, over
    assert len(spans) == 36 and max(v[0] for v in spans.values()) < 60 * 1024
    # the formula of policy.hpp policy_vjp_lds_bytes, and its limits
    lds = lambda hidden, elem: sum(hidden) * 64 * elem
    assert lds((64, 64, 64), 4) == 48 * 1024 and lds((64, 64, 64), 8) == 96 * 1024 and lds((), 8) == 0
    assert lds(hp.NETS["N1"], 4) == 16 * 64 * 4 and lds(hp.NETS["N2"], 8) == 131 * 64 * 8 <= 96 * 1024


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _record(widths=(2, 5, 1), **kw):
    ptrs = (ctypes.c_void_p * 8)(*([64] * 8))
    w = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*widths)
    pol = _native.Policy(64, len(widths) - 1, _native.ACT_TANH, w, None, -1.0, 1.0)
    for k in [k for k in kw if k.startswith("policy_")]:
        setattr(pol, k[len("policy_"):], kw.pop(k))
    r = _native.PolicyVjp(pol, 64, ctypes.addressof(ptrs), 64, None, None, None, None, None, ctypes.addressof(ptrs), 64)
    r._keep = ptrs
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(env=0, solver=0, dtype=0, B=4, K=3, sub=1, props=None, control=None, opts=None, rec=None, no_props=False, no_rec=False):
    lib = _native.lib()
    p = props if props is not None else _native.Props()
    r = rec if rec is not None else _record()
    rc = lib.excenv_sim_policy_vjp(env, solver, dtype, i64(B), i64(K), i32(sub), None if no_props else ctypes.byref(p),
                                   None if control is None else ctypes.byref(control), dbl(1e-4), dbl(1e-4),
                                   None if no_rec else ctypes.byref(r), None if opts is None else ctypes.byref(opts), None)
    return rc, lib.excenv_last_error().decode()


def test_refusals_come_back_by_code_and_whole_message_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    assert _call(no_props=True) == (ENULL, f"{FN}: props is NULL")
    assert _call(no_rec=True) == (ENULL, f"{FN}: call is NULL")
    table = [
        # the policy inside the record: excenv_sim_policy's refusals under this entry's name
        (dict(policy_params=None), ENULL, "policy->params is NULL"),
        (dict(policy_n_layers=5), EINVAL, "policy->n_layers must be 1 .. 4 (got 5)"),
        (dict(widths=(3, 5, 1)), EINVAL, "policy->widths must run from the observation width 2 to the action width 1 (got 3 .. 1)"),
        (dict(widths=(2, 65, 1)), EINVAL, "policy->widths[1] must be 1 .. 64 (got 65)"),
        (dict(policy_activation=2), EINVAL, "policy->activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got 2)"),
        (dict(policy_clip_lo=1.0, policy_clip_hi=-1.0), EINVAL,
         "policy->clip_lo = 1 and policy->clip_hi = -1 are not an interval (-inf / +inf: no clamp)"),
        (dict(policy_clip_lo=float("nan")), EINVAL, "policy->clip_lo = nan and policy->clip_hi = 1 are not an interval (-inf / +inf: no clamp)"),
        # the record
        (dict(obs_traj=None), ENULL, "call->obs_traj (the policy is evaluated again on the saved observation rows) is NULL"),
        (dict(state_traj=None), ENULL, "call->state_traj (the reverse pass reads the saved rows) is NULL"),
        (dict(actions=None), ENULL, "call->actions is NULL"),
        (dict(grad_state0=None), ENULL, "call->grad_state0 is NULL"),
        (dict(grad_raw=None), ENULL, "call->grad_raw is NULL"),
    ]
    for kw, code, text in table:
        assert _call(rec=_record(**kw)) == (code, f"{FN}: {text}"), kw
    assert _call(sub=3, rec=_record(reset=64)) == (
        EINVAL, f"{FN}: call->reset needs substeps == 1 (one solver step per action, as excenv_sim_policy_episodes; got 3)")
    assert _call(K=2 ** 30, sub=2) == (EINVAL, f"{FN}: K * substeps = 1073741824 * 2 rows exceed one launch")
    # K == 0 needs neither the actions nor grad_raw; B == 0 ends every valid call without a launch (the empty batch)
    assert _call(B=0, K=0, rec=_record(actions=None, grad_raw=None))[0] == 0
    assert _call(B=0)[0] == 0 and _call(B=0, sub=1, rec=_record(reset=64))[0] == 0
    assert _call(B=0, K=2 ** 30 - 1, sub=2)[0] == 0
    assert _call(B=0, opts=_native.LaunchOpts(1, 0, 0, 0))[0] == 0
    # PMSM with substeps != 1, a forced width that cannot be had
    pm = _record(widths=(8, 2))
    assert _call(env=5, sub=2, rec=pm) == (EINVAL, f"{FN}: PMSM: obs_stepsize must equal action_stepsize (substeps = 2; reference pmsm_env.py:787)")
    for v in (2, 4):
        assert _call(opts=_native.LaunchOpts(v, 0, 0, 0)) == (
            EINVAL, f"{FN}: opts.envs_per_lane = {v} is not available (this kernel has the one-environment-per-lane form only)")
    # the saturated PMSM, per-environment property arrays: the messages of every reverse entry
    p = _native.Props()
    lut = _native.PmsmLut(4, 4, 64, 64, 64)
    p.pmsm_lut = ctypes.pointer(lut)
    assert _call(env=5, props=p, rec=pm) == (EUNSUPPORTED, f"{FN}: the saturated PMSM (pmsm_lut) has no reverse mode")
    for field in ("static_params", "state_max", "action_min"):
        p = _native.Props()
        getattr(p, field)[0].per_env = 64
        assert _call(props=p) == (EUNSUPPORTED, f"{FN}: per-environment property arrays are not supported (broadcast properties only)"), field
    # bad values; only the count of the control record is read
    assert _call(env=9)[0] == EINVAL and _call(solver=3)[0] == EINVAL and _call(dtype=2)[0] == EINVAL and _call(B=-1)[0] == EINVAL
    assert _call(K=-1) == (EINVAL, f"{FN}: bad K=-1 or substeps=1") and _call(sub=0) == (EINVAL, f"{FN}: bad K=3 or substeps=0")
    c = _native.Control()
    c.n_control = 9
    assert _call(control=c) == (EINVAL, f"{FN}: bad n_control 9")
    c.n_control = 1
    assert _call(control=c) == (EINVAL, f"{FN}: policy->widths must run from the observation width 3 to the action width 1 (got 2 .. 1)")
    assert _call(B=0, control=c, rec=_record(widths=(3, 5, 1)))[0] == 0


def test_bytes_function_is_the_formula():
    lib = _native.lib()
    for env in range(6):
        S, A, O, _ = _native.env_dims(env)
        for dtype, w in ((_native.F32, 4), (_native.F64, 8)):
            for nc, sub, go, gs, ga in itertools.product((0, 2), (1, 3), (0, 1), (0, 1), (0, 1)):
                want = w * (sub * (S + go * O + gs * S) + (O + nc) + A * (2 + ga))
                assert lib.excenv_sim_policy_vjp_bytes(env, dtype, nc, sub, go, gs, ga, 0) == want, (env, dtype, nc, sub, go, gs, ga)
                if sub == 1:
                    assert lib.excenv_sim_policy_vjp_bytes(env, dtype, nc, sub, go, gs, ga, 1) == want + 1
    bad = [(17, 0, 0, 1, 0, 0, 0, 0), (0, 5, 0, 1, 0, 0, 0, 0), (0, 0, 9, 1, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 3, 0, 0, 0, 1)]
    assert all(lib.excenv_sim_policy_vjp_bytes(*a) == -1 for a in bad)


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def _policy(widths=(2, 5, 1), activation="tanh", dtype=torch.float32, seed=3):
    g = torch.Generator().manual_seed(seed)
    W = [torch.randn(d, n, generator=g, dtype=dtype) for n, d in zip(widths[:-1], widths[1:])]
    b = [torch.randn(d, generator=g, dtype=dtype) for d in widths[1:]]
    return MLPPolicy(W, b, activation)


def test_python_refuses_by_name_what_the_reverse_mode_does_not_do():
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    _, state = env.vmap_reset()
    policy = _policy()
    policy.params.requires_grad_()
    # the default keyword: exactly the refusal of before
    env.differentiable = True
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy: env.differentiable with an input that requires grad: there is no reverse mode"):
        env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau)
    env.differentiable = False
    env.store_state_trajectory = False
    with pytest.raises(ValueError, match=r"vmap_sim_ahead_policy\(differentiable=True\): store_state_trajectory=False"):
        env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau, differentiable=True)
    env.store_state_trajectory = True
    acts = torch.zeros(4, 3, 1)
    for layout in ("env_major", "tiled"):
        env.traj_layout = layout
        with pytest.raises(ValueError, match=f"traj_layout='{layout}'"):
            env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau, differentiable=True)
        with pytest.raises(ValueError, match=f"vmap_sim_ahead_policy_vjp: traj_layout='{layout}'"):
            env.vmap_sim_ahead_policy_vjp(policy, None, None, acts, env.tau, env.tau)
    env.traj_layout = "lane_major"
    env.sim_ahead_semantics = "ahead_accumulated_t"
    with pytest.raises(ValueError, match="ahead_accumulated_t"):
        env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau, differentiable=True)
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy_vjp: sim_ahead_semantics='ahead_accumulated_t'"):
        env.vmap_sim_ahead_policy_vjp(policy, None, None, acts, env.tau, env.tau)
    env.sim_ahead_semantics = "ahead"
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy_vjp: `states` is None"):
        env.vmap_sim_ahead_policy_vjp(policy, None, None, acts, env.tau, env.tau)
    # per-environment properties, a static parameter that requires grad
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", static_params={"g": torch.full((4,), 9.81), "l": 1.0, "m": 1.0})
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match=r"vmap_sim_ahead_policy\(differentiable=True\): per-environment"):
        env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau, differentiable=True)
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy_vjp: per-environment"):
        env.vmap_sim_ahead_policy_vjp(policy, None, None, acts, env.tau, env.tau)
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu",
                                            static_params={"g": 9.81, "l": torch.tensor(1.0, requires_grad=True), "m": 1.0})
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match="static parameter 'l' requires grad"):
        env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau, differentiable=True)
    assert env.last_policy_vjp_launch == ""


def test_saturated_pmsm_is_refused_by_name():
    from helpers_feedback import saturated_env

    env, _, _, _ = saturated_env(4, torch.float32, "euler", "cpu")
    _, state = env.vmap_reset()
    policy = _policy((8, 3, 2))
    policy.params.requires_grad_()
    with pytest.raises(ValueError, match=r"vmap_sim_ahead_policy\(differentiable=True\): the saturated PMSM has no reverse mode"):
        env.vmap_sim_ahead_policy(state, policy, 3, env.tau, env.tau, differentiable=True)
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy_vjp: the saturated PMSM has no reverse mode"):
        env.vmap_sim_ahead_policy_vjp(policy, None, None, torch.zeros(4, 3, 2), env.tau, env.tau)


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("net", sorted(hp.NETS))
def test_torch_forward_is_the_numpy_policy(net, activation):
    """fp64, 1e-13 of the largest output: the two differ by the order of the sums only"""
    rng = np.random.default_rng(17)
    widths = (5,) + hp.NETS[net] + (2,)
    W = [rng.normal(0, 1 / np.sqrt(n), (d, n)) for n, d in zip(widths[:-1], widths[1:])]
    b = [rng.uniform(-0.1, 0.1, d) for d in widths[1:]]
    rows = rng.uniform(-1, 1, (37, 5))
    policy = MLPPolicy(W, b, activation)
    assert policy.params.dtype == torch.float64
    _, raw, _ = hp.mlp_np(rows, W, b, activation, None, None)
    got = policy.torch_forward(torch.as_tensor(rows))
    d = float(np.max(np.abs(got.numpy() - raw))) / float(np.max(np.abs(raw)))
    print(f"{net} {activation}: {d:.3e}")
    assert got.shape == (37, 2) and d <= 1e-13
    # `params`: another tensor of the same layout, with a graph
    p = (2.0 * policy.params).requires_grad_()
    y = policy.torch_forward(torch.as_tensor(rows)[None], p)
    assert y.shape == (1, 37, 2) and torch.autograd.grad(y.sum(), p)[0].shape == p.shape


def test_from_torch_track_reaches_the_modules_grad():
    nn = torch.nn
    module = nn.Sequential(nn.Linear(3, 4), nn.Tanh(), nn.Linear(4, 2)).double()
    plain = MLPPolicy.from_torch(module)
    assert not plain.params.requires_grad and plain.params.grad_fn is None  # the default: a detached copy
    policy = MLPPolicy.from_torch(module, track=True)
    assert policy.params.grad_fn is not None and torch.equal(policy.params.detach(), plain.params) and policy.widths == (3, 4, 2)
    rows = torch.randn(6, 3, dtype=torch.float64)
    w = torch.randn(6, 2, dtype=torch.float64)
    (policy.torch_forward(rows) * w).sum().backward()
    want = torch.autograd.grad((module(rows) * w).sum(), list(module.parameters()))
    for p, g in zip(module.parameters(), want):
        assert p.grad is not None and torch.allclose(p.grad, g, rtol=1e-12, atol=1e-14)
    # a snapshot: an optimiser step changes the module, not the policy
    with torch.no_grad():
        module[0].weight.add_(1.0)
    assert torch.equal(policy.params.detach(), plain.params)


# ---- the twin and its inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_twin_forward_is_the_oracles_policy_loop(env_name, deadtime, solver):
    """Network N1, tanh: within 1e-12 of full scale, wrapped angles on the circle"""
    _, _, _, _, out = hv.main_twin(env_name, deadtime, solver, "N1", "tanh")
    want = hp.oracle_case(env_name, deadtime, solver, "N1", "tanh")
    d = np.abs(out["obs"].detach().numpy() - want["obs"])
    for c in ANGLE_OBS.get(env_name, []):
        d[..., c] = np.minimum(d[..., c], np.abs(2.0 - d[..., c]))
    dist = float(d.max()) / float(np.max(np.abs(want["obs"])))
    da = float(np.max(np.abs(out["actions"].detach().numpy() - want["actions"])))
    print(f"{env_name} deadtime {deadtime} {solver}: observations {dist:.3e}, actions {da:.3e}")
    assert dist <= 1e-12 and da <= 1e-12


@pytest.mark.parametrize("activation", hp.ACTIVATIONS)
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_input_conditions_of_the_main_cases(env_name, deadtime, solver, activation):
    """On the twin alone, network N1: at most KINK_CAP of the environments are excluded (within KINK_MARGIN of a model kink or a
    clamp bound, or with a ReLU pre-activation below RELU_MARGIN), and the cotangent group `grad_actions alone` reaches the initial
    state — only through the transposed network — in at least 90 % of the environments."""
    spec, inp, twin, lv, out = hv.main_twin(env_name, deadtime, solver, "N1", activation)
    keep = hv.keep_mask(twin, out, activation)
    excluded = 1.0 - float(np.mean(keep))
    B, K, A = hv.B_MAIN, hv.K_MAIN, hp.action_dim(env_name)
    g = hv.twin_grads(lv, out, [dict(actions=np.random.default_rng(5).normal(size=(B, K, A)))])[0]
    reached = float(np.mean(np.any(np.stack(g["state0"]) != 0, axis=0)))
    print(f"{env_name} deadtime {deadtime} {solver} {activation}: excluded {excluded:.4f}, clamp active {out['clamped']:.3f}, "
          f"grad_actions alone reaches state0 in {reached:.3f} of the environments")
    assert excluded <= hv.KINK_CAP
    assert reached >= 0.9
