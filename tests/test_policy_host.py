"""Host side of the policy rollouts (no GPU): the header declares excenv_sim_policy and _native mirrors it, the entry point refuses by
code and whole message what it does not do before any launch, every built sim_policy_kernel instantiation is free of scratch memory,
the numpy restatement of the contract and the exact CPU fused multiply-add are what they say, the test inputs clamp some but not most
actions and leave ReLU neither dead nor transparent on the float64 oracle loop, `MLPPolicy.from_torch` round-trips parameters, and
`vmap_sim_ahead_policy` raises the named exceptions on CPU environments."""
import ctypes
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget
import helpers_policy as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL = -1, -2
MODELS = ["Pendulum", "MassSpringDamper", "CartPole", "Acrobot", "FluidTank", "Pmsm", "PmsmSat"]


def test_header_declares_native_mirrors_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_sim_policy\s*\(", hdr)
    assert re.search(r"\}\s*excenv_policy_t\s*;", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # an addition: a binder probes for the symbol
    assert re.search(r"#define\s+EXCENV_POLICY_MAX_LAYERS\s+4\b", hdr) and re.search(r"#define\s+EXCENV_POLICY_MAX_WIDTH\s+64\b", hdr)
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_sim_policy")
    assert lib.excenv_abi_version() == 7 and _native.ABI_VERSION == 7
    assert len(_native.PROTOTYPES["excenv_sim_policy"][1]) == 18
    assert _native.STRUCTS[_native.Policy] == "excenv_policy_t"
    assert [f[0] for f in _native.Policy._fields_] == ["params", "n_layers", "activation", "widths", "noise", "clip_lo", "clip_hi"]
    assert (_native.POLICY_MAX_LAYERS, _native.POLICY_MAX_WIDTH, _native.ACT_RELU, _native.ACT_TANH) == (4, 64, 0, 1)


# ---- refusals: fake 16-byte aligned addresses everywhere, nothing may reach a launch ----------------------------------------------
def _call(env=0, B=4, K=2, substeps=1, policy="default", null=None, epl=0, lut=False, widths=(2, 8, 1), n_layers=None, activation=1,
          n_control=0, **pol):
    """One excenv_sim_policy call (pendulum: O = 2, A = 1). null: the argument (or policy field) passed as NULL; pol: policy fields"""
    lib = _native.lib()
    props = _native.Props()
    keep = []
    if lut:
        keep.append(_native.PmsmLut(4, 4, 64, 64, 64))
        props.pmsm_lut = ctypes.pointer(keep[0])
    ptrs = lambda: (ctypes.c_void_p * 8)(*([64] * 8))
    a = dict(state_in=ptrs(), obs_traj=vp(64), state_traj=ptrs(), last_state=ptrs(), actions_out=vp(64))
    f = dict(params=64, noise=None, clip_lo=-1.0, clip_hi=1.0)
    f.update(pol)
    if null in a:
        a[null] = None
    elif null in f:
        f[null] = None
    elif null is not None:  # "last_state[1]": one entry of a pointer array
        name, j = null[:-3], int(null[-2])
        a[name][j] = None
    w = (ctypes.c_int32 * 5)(*(tuple(widths) + (0,) * (5 - len(widths))))
    p = _native.Policy(f["params"], len(widths) - 1 if n_layers is None else n_layers, activation, w, f["noise"], f["clip_lo"], f["clip_hi"])
    control = None
    if n_control:
        control = _native.Control(n_control, (ctypes.c_int32 * 8)(*([0] * 8)), (ctypes.c_void_p * 8)(*([64] * 8)), (ctypes.c_void_p * 8)())
    opts = _native.LaunchOpts(epl, 0, 0, 0)
    rc = lib.excenv_sim_policy(env, 0, 0, i64(B), i64(K), i32(substeps), ctypes.byref(props), None if control is None else ctypes.byref(control),
                               dbl(1e-4), dbl(1e-4), a["state_in"], None if policy is None else ctypes.byref(p), a["obs_traj"],
                               a["state_traj"], a["last_state"], a["actions_out"], ctypes.byref(opts), None)
    return rc, lib.excenv_last_error().decode()


_CLIP = "excenv_sim_policy: policy->clip_lo = %s and policy->clip_hi = %s are not an interval (-inf / +inf: no clamp)"
# what the call is made with, return code, the whole message
REFUSALS = [
    (dict(policy=None), ENULL, "excenv_sim_policy: policy is NULL"),
    (dict(null="params"), ENULL, "excenv_sim_policy: policy->params is NULL"),
    (dict(null="obs_traj"), ENULL, "excenv_sim_policy: obs_traj is NULL"),
    (dict(null="last_state"), ENULL, "excenv_sim_policy: last_state is NULL"),
    (dict(null="state_in"), ENULL, "excenv_sim_policy: state_in is NULL"),
    (dict(null="last_state[1]"), ENULL, "excenv_sim_policy: state pointer 1 is NULL"),
    (dict(null="state_in[0]"), ENULL, "excenv_sim_policy: state pointer 0 is NULL"),
    (dict(null="state_traj[0]"), ENULL, "excenv_sim_policy: state_traj pointer 0 is NULL"),
    (dict(n_layers=0), EINVAL, "excenv_sim_policy: policy->n_layers must be 1 .. 4 (got 0)"),
    (dict(n_layers=5), EINVAL, "excenv_sim_policy: policy->n_layers must be 1 .. 4 (got 5)"),
    (dict(n_layers=-1), EINVAL, "excenv_sim_policy: policy->n_layers must be 1 .. 4 (got -1)"),
    (dict(widths=(2, 65, 1)), EINVAL, "excenv_sim_policy: policy->widths[1] must be 1 .. 64 (got 65)"),
    (dict(widths=(2, 8, 0, 1)), EINVAL, "excenv_sim_policy: policy->widths[2] must be 1 .. 64 (got 0)"),
    (dict(widths=(2, 64, 64, -3, 1)), EINVAL, "excenv_sim_policy: policy->widths[3] must be 1 .. 64 (got -3)"),
    (dict(widths=(3, 8, 1)), EINVAL,
     "excenv_sim_policy: policy->widths must run from the observation width 2 to the action width 1 (got 3 .. 1)"),
    (dict(widths=(2, 8, 2)), EINVAL,
     "excenv_sim_policy: policy->widths must run from the observation width 2 to the action width 1 (got 2 .. 2)"),
    (dict(widths=(2, 1), n_control=2), EINVAL,
     "excenv_sim_policy: policy->widths must run from the observation width 4 to the action width 1 (got 2 .. 1)"),
    (dict(activation=2), EINVAL, "excenv_sim_policy: policy->activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got 2)"),
    (dict(activation=-1), EINVAL, "excenv_sim_policy: policy->activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got -1)"),
    (dict(clip_lo=0.5, clip_hi=0.25), EINVAL, _CLIP % ("0.5", "0.25")),
    (dict(clip_lo=math.nan), EINVAL, _CLIP % ("nan", "1")),
    (dict(clip_hi=math.nan), EINVAL, _CLIP % ("-1", "nan")),
    (dict(env=5, substeps=2, widths=(8, 2)), EINVAL,
     "excenv_sim_policy: PMSM: obs_stepsize must equal action_stepsize (substeps = 2; reference pmsm_env.py:787)"),
    (dict(env=5, substeps=3, lut=True, widths=(8, 4, 2)), EINVAL,
     "excenv_sim_policy: PMSM: obs_stepsize must equal action_stepsize (substeps = 3; reference pmsm_env.py:787)"),
    (dict(epl=2), EINVAL,
     "excenv_sim_policy: opts.envs_per_lane = 2 is not available (this kernel has the one-environment-per-lane form only)"),
    (dict(epl=4), EINVAL,
     "excenv_sim_policy: opts.envs_per_lane = 4 is not available (this kernel has the one-environment-per-lane form only)"),
    (dict(epl=3), EINVAL, "excenv_sim_policy: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)"),
    (dict(K=-1), EINVAL, "excenv_sim_policy: bad K=-1 or substeps=1"),
    (dict(substeps=0), EINVAL, "excenv_sim_policy: bad K=2 or substeps=0"),
    (dict(B=-1), EINVAL, "excenv_sim_policy: bad batch size -1"),
    (dict(env=7), EINVAL, "excenv_sim_policy: bad env id 7"),
    (dict(env=0, lut=True), EINVAL, "pmsm_lut is only valid for EXCENV_PMSM"),
]


def test_the_pmsm_refusals_use_its_widths():
    assert (hp.obs_width("pmsm"), hp.action_dim("pmsm")) == (8, 2)


@pytest.mark.parametrize("how,rc,message", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in REFUSALS])
def test_the_refusal_comes_back_by_code_and_whole_message(how, rc, message):
    assert _call(**how) == (rc, message)


def test_an_empty_batch_is_ok_without_a_launch():
    """B == 0: nothing to do — and no GPU here, so a launch would have come back as EXCENV_EHIP. (K == 0 launches: row 0 only; the
    GPU suite covers it.)"""
    assert _call(B=0)[0] == 0
    assert _call(B=0, K=0, widths=(2, 1))[0] == 0
    assert _call(B=0, epl=1, widths=(2, 64, 64, 64, 1), activation=0)[0] == 0


def test_sim_policy_kernels_exist_and_use_no_scratch():
    """tools/loop_code_size.py kernel_resources on the built library: the 42 instantiations (seven models, the saturated PMSM
    included, x three solvers x two element types) are all there and none has a private segment."""
    res, spans = budget("sim_policy_kernel")
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"sim_policy_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]} loop {spans[hit[0]][0]} B of {spans[hit[0]][1]} B")
    assert len(res) == 42, len(res)
    assert all(v["scratch"] == 0 for v in res.values()), {k: v for k, v in res.items() if v["scratch"]}
    assert all(v["lds"] == 0 for v in res.values())  # no static LDS: the launch sizes it by the call's widest hidden layer
    assert max(v[0] for v in spans.values()) < 60 * 1024  # the trajectory loop stays inside the instruction cache


# ---- the references the GPU suite rests on -----------------------------------------------------------------------------------------
def test_policy_restatement_is_the_written_contract():
    """mlp_np against the formula spelled out entry by entry: one environment, 3 -> 2 -> 2, every value a small dyadic number"""
    ob = np.array([[0.5, -0.25, 2.0]])
    W = [np.array([[1.0, 2.0, 0.5], [-4.0, 0.0, 0.25]]), np.array([[2.0, -1.0], [0.5, 8.0]])]
    b = [np.array([0.125, 1.0]), np.array([-0.5, 0.25])]
    y1 = [0.125 + 0.5 - 0.5 + 1.0, 1.0 - 2.0 + 0.0 + 0.5]  # 1.125, -0.5
    a, raw, pre = hp.mlp_np(ob, W, b, "relu", np.array([[0.25, -3.0]]), (-1.0, 1.0))
    assert pre[0].tolist() == [y1]
    assert raw.tolist() == [[0.25 + (-0.5 + 2.0 * 1.125 - 0.0), -3.0 + (0.25 + 0.5 * 1.125 + 0.0)]]  # ReLU: -0.5 -> 0
    assert a.tolist() == [[1.0, -1.0]]
    a, raw, _ = hp.mlp_np(ob, W, b, "relu", None, None)
    assert a.tolist() == raw.tolist() == [[1.75, 0.8125]]
    a, raw, _ = hp.mlp_np(ob, W, b, "tanh", None, None)
    t = np.tanh(np.array(y1))
    assert raw.tolist() == [[2.0 * t[0] + -0.5 + -1.0 * t[1], (0.5 * t[0] + 0.25) + 8.0 * t[1]]]
    # no hidden layer; a NaN passes the clamp
    a, raw, pre = hp.mlp_np(ob, W[:1], b[:1], "relu", None, (-1.0, 1.0))
    assert pre == [] and raw.tolist() == [y1] and a.tolist() == [[1.0, -0.5]]
    a, _, _ = hp.mlp_np(np.array([[np.nan, 0.0, 0.0]]), W[:1], b[:1], "relu", None, (-1.0, 1.0))
    assert np.isnan(a).all()
    # the exact forms agree on exactly representable values, in their dtypes
    for dt in (np.float32, np.float64):
        a, raw, _ = hp.mlp_np(ob, W, b, "relu", np.array([[0.25, -3.0]]), (-1.0, 1.0), exact=dt)
        assert a.dtype == dt and a.tolist() == [[1.0, -1.0]] and raw.tolist() == [[2.0, -2.1875]]
    # the bound: zero width at the observations, grows with every layer, and holds the float32 evaluation of the same network
    rng = np.random.default_rng(3)
    obs = rng.uniform(-1, 1, (5, 2, 3)).astype(np.float32).astype(np.float64)
    Wr = [rng.normal(0, 0.6, (4, 3)).astype(np.float32).astype(np.float64), rng.normal(0, 0.5, (2, 4)).astype(np.float32).astype(np.float64)]
    br = [rng.uniform(-0.1, 0.1, 4).astype(np.float32).astype(np.float64), rng.uniform(-0.1, 0.1, 2).astype(np.float32).astype(np.float64)]
    want, bound = hp.policy_bounds(obs, Wr, br, "relu", None, None, np.float32)
    got = np.stack([hp.mlp_np(obs[:, k], Wr, br, "relu", None, None, exact=np.float32)[0] for k in range(2)], axis=1).astype(np.float64)
    assert np.all(bound > 0) and np.all(np.abs(got - want) <= bound) and np.any(got != want)


def _is_nearest(x, r, dtype):
    """Is the float r (of dtype) a round-to-nearest-even result of the exact Fraction x?"""
    r = dtype(r)
    d = abs(x - Fraction(float(r)))
    for n in (np.nextafter(r, dtype(np.inf)), np.nextafter(r, dtype(-np.inf))):
        dn = abs(x - Fraction(float(n)))
        if dn < d:
            return False
        if dn == d and d != 0:  # a tie: the even mantissa wins
            bits = int(np.array(r).view(np.int32 if dtype is np.float32 else np.int64))
            if bits & 1:
                return False
    return True


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_the_cpu_fused_multiply_add_is_exact(dtype):
    """helpers_policy.fma_exact against fractions.Fraction on 10^5 random triples: a third with independent exponents, a third with
    c close to -a * b (cancellation: the low part of the product decides), a third where a * b + c is a near-tie of the rounding"""
    rng = np.random.default_rng(11)
    n = 100_000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 9, n)).astype(dtype)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-8, 9, n)).astype(dtype)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 13, n)).astype(dtype)
    third = n // 3
    prod = (a.astype(np.float64) * b.astype(np.float64))
    c[third:2 * third] = (-prod[third:2 * third] * (1 + rng.integers(-3, 4, third) * np.finfo(dtype).eps)).astype(dtype)
    # near-ties: c a few hundred ulps of the product, so that the product's low half lands next to a rounding boundary of the sum
    c[2 * third:] = (prod[2 * third:] * rng.integers(1, 512, n - 2 * third)).astype(dtype)
    got = hp.fma_exact(a, b, c, dtype)
    assert got.dtype == dtype
    bad = 0
    for j in range(n):
        x = Fraction(float(a[j])) * Fraction(float(b[j])) + Fraction(float(c[j]))
        bad += not _is_nearest(x, got[j], dtype)
    assert bad == 0, bad
    # and it is not the unfused form: some results differ from round(round(a * b) + c)
    assert np.any(got != (a * b + c).astype(dtype))


# ---- the input condition, on the oracle alone: neither "never clamps" nor "always clamps", ReLU neither dead nor transparent ----------
MAIN_NETS = [("N1", "relu"), ("N1", "tanh"), ("N2", "relu"), ("N2", "tanh"), ("N0", "relu")]


@pytest.mark.parametrize("net,activation", MAIN_NETS, ids=[f"{n}-{a}" for n, a in MAIN_NETS])
@pytest.mark.parametrize("solver", hp.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hp.CASES)
def test_the_inputs_clamp_some_but_not_most_actions_on_the_oracle(env_name, deadtime, solver, net, activation):
    r = hp.oracle_case(env_name, deadtime, solver, net, activation)
    print(f"{env_name} deadtime {deadtime} {solver} {net} {activation}: clamped share {r['clamped']:.3f}, negative hidden "
          f"pre-activations {r['negative']:.3f}")
    assert 0.05 < r["clamped"] < 0.60
    assert np.all(np.isfinite(r["obs"])) and np.all(np.isfinite(r["actions"]))
    assert r["obs"].shape == (hp.B_MAIN, hp.K_MAIN * hp.substeps_of(env_name) + 1, hp.obs_width(env_name))
    if hp.NETS[net]:
        assert 0.10 <= r["negative"] <= 0.90


# ---- MLPPolicy ---------------------------------------------------------------------------------------------------------------------
def test_from_torch_round_trips_and_refuses_by_name():
    nn = torch.nn
    torch.manual_seed(5)
    for act, name in ((nn.Tanh, "tanh"), (nn.ReLU, "relu")):
        mod = nn.Sequential(nn.Linear(4, 11), act(), nn.Linear(11, 5), act(), nn.Linear(5, 2)).double()
        pol = excenvs.MLPPolicy.from_torch(mod)
        assert pol.widths == (4, 11, 5, 2) and pol.activation == name and pol.n_layers == 3
        assert pol.params.dtype == torch.float64 and pol.params.numel() == 11 * 5 + 5 * 12 + 2 * 6 and not pol.params.requires_grad
        for (W, b), lin in zip(pol.layers(), [mod[0], mod[2], mod[4]]):
            assert torch.equal(W, lin.weight.detach()) and torch.equal(b, lin.bias.detach())
        x = torch.randn(7, 4, dtype=torch.float64)
        a, _, _ = hp.mlp_np(x.numpy(), [w.numpy() for w, _ in pol.layers()], [b.numpy() for _, b in pol.layers()], name, None, None)
        np.testing.assert_allclose(a, mod(x).detach().numpy(), rtol=0, atol=1e-14)
    one = excenvs.MLPPolicy.from_torch(nn.Sequential(nn.Linear(3, 2)))
    assert one.widths == (3, 2) and one.n_layers == 1 and one.activation == "tanh" and one.params.dtype == torch.float32
    assert excenvs.MLPPolicy.from_torch(nn.Sequential(nn.Linear(3, 2)), dtype=torch.float64).on("cpu", torch.float64).dtype == torch.float64
    direct = excenvs.MLPPolicy([np.ones((2, 3))], [np.zeros(2)], "relu")
    assert direct.widths == (3, 2) and direct.params.tolist() == [1.0] * 6 + [0.0] * 2
    for bad, message in (
            (nn.Linear(3, 2), "needs an nn.Sequential of Linear layers, got Linear"),
            (nn.Sequential(nn.Linear(3, 4), nn.Tanh()), "a Linear layer first and last"),
            (nn.Sequential(nn.Tanh(), nn.Linear(3, 4), nn.Tanh()), "module 0 must be nn.Linear, got Tanh"),
            (nn.Sequential(nn.Linear(3, 4), nn.Sigmoid(), nn.Linear(4, 1)), "module 1 must be nn.Tanh or nn.ReLU, got Sigmoid"),
            (nn.Sequential(nn.Linear(3, 4), nn.Tanh(), nn.Linear(4, 4), nn.ReLU(), nn.Linear(4, 1)), "nn.Tanh and nn.ReLU mixed"),
            (nn.Sequential(nn.Linear(3, 4, bias=False), nn.Tanh(), nn.Linear(4, 1)), r"module 0: nn.Linear\(bias=False\) is not supported"),
            (nn.Sequential(nn.Linear(3, 65), nn.Tanh(), nn.Linear(65, 1)), "hidden layer 1 has 65 units; 1 to 64 are supported"),
            (nn.Sequential(*[m for _ in range(4) for m in (nn.Linear(3, 3), nn.Tanh())], nn.Linear(3, 1)),
             "5 Linear layers; at most 4 are supported"),
            (nn.Sequential(nn.Linear(3, 4), nn.Tanh(), nn.Dropout(), nn.Linear(4, 1)), "a Linear layer first and last")):
        with pytest.raises(ValueError, match="MLPPolicy.from_torch: .*" + message):
            excenvs.MLPPolicy.from_torch(bad)
    with pytest.raises(ValueError, match="MLPPolicy: activation='gelu'"):
        excenvs.MLPPolicy([np.ones((2, 3))], [np.zeros(2)], "gelu")
    with pytest.raises(AssertionError, match="layer 2 reads 5 inputs, but layer 1 has 4 outputs"):
        excenvs.MLPPolicy([np.ones((4, 3)), np.ones((1, 5))], [np.zeros(4), np.zeros(1)])
    with pytest.raises(AssertionError, match="hidden layer 1 has 65 units"):
        excenvs.MLPPolicy([np.ones((65, 3)), np.ones((1, 65))], [np.zeros(65), np.zeros(1)])
    with pytest.raises(AssertionError, match="1 to 4 linear layers"):
        excenvs.MLPPolicy([], [])


# ---- Python argument faults (CPU environments: raised before anything touches a device) ---------------------------------------------
def _cpu_env(**kw):
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", **kw)
    _, state = env.vmap_reset()
    return env, state


def _policy(widths=(2, 3, 1), **kw):
    return excenvs.MLPPolicy([torch.zeros(d, n) for n, d in zip(widths[:-1], widths[1:])], [torch.zeros(d) for d in widths[1:]], **kw)


def test_python_refuses_by_name_what_a_policy_rollout_does_not_do():
    env, state = _cpu_env()
    pol = _policy()
    for layout in ("env_major", "tiled"):
        env.traj_layout = layout
        with pytest.raises(ValueError, match=f"vmap_sim_ahead_policy: traj_layout='{layout}'"):
            env.vmap_sim_ahead_policy(state, pol, 3, env.tau, env.tau)
    env.traj_layout = "lane_major"
    env.sim_ahead_semantics = "ahead_accumulated_t"
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy: sim_ahead_semantics='ahead_accumulated_t'"):
        env.vmap_sim_ahead_policy(state, pol, 3, env.tau, env.tau)
    env.sim_ahead_semantics = "ahead"
    env.differentiable = True
    with pytest.raises(ValueError, match="vmap_sim_ahead_policy: env.differentiable with an input that requires grad"):
        env.vmap_sim_ahead_policy(state, pol, 3, env.tau, env.tau, noise=torch.zeros(4, 3, 1, requires_grad=True))
    live = _policy()
    live.params.requires_grad_()
    with pytest.raises(ValueError, match="env.differentiable with an input that requires grad"):
        env.vmap_sim_ahead_policy(state, live, 3, env.tau, env.tau)
    state.physical_state.theta = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError, match="env.differentiable with an input that requires grad"):
        env.vmap_sim_ahead_policy(state, pol, 3, env.tau, env.tau)
    assert env.last_policy_launch == ""


def test_python_shape_faults_are_assertion_errors_with_a_message():
    env, state = _cpu_env()
    ok = _policy()
    with pytest.raises(AssertionError, match="policy needs to be an MLPPolicy, but Tensor is given"):
        env.vmap_sim_ahead_policy(state, torch.zeros(1, 2), 3, env.tau, env.tau)
    with pytest.raises(AssertionError, match=r"observation width 2 to the action width 1, but its widths are \(3, 3, 1\)"):
        env.vmap_sim_ahead_policy(state, _policy((3, 3, 1)), 3, env.tau, env.tau)
    with pytest.raises(AssertionError, match=r"observation width 2 to the action width 1, but its widths are \(2, 2\)"):
        env.vmap_sim_ahead_policy(state, _policy((2, 2)), 3, env.tau, env.tau)
    with pytest.raises(AssertionError, match="The noise needs to have three dimensions"):
        env.vmap_sim_ahead_policy(state, ok, 3, env.tau, env.tau, noise=torch.zeros(4, 3))
    with pytest.raises(AssertionError, match="n_actions is 5, but the noise has 3 action rows"):
        env.vmap_sim_ahead_policy(state, ok, 5, env.tau, env.tau, noise=torch.zeros(4, 3, 1))
    with pytest.raises(AssertionError, match="n_actions is needed"):
        env.vmap_sim_ahead_policy(state, ok, None, env.tau, env.tau)
    with pytest.raises(AssertionError, match="clip needs to be"):
        env.vmap_sim_ahead_policy(state, ok, 3, env.tau, env.tau, clip=(1.0, -1.0))
    with pytest.raises(AssertionError, match="action stepsize should be greater or equal"):
        env.vmap_sim_ahead_policy(state, ok, 3, env.tau, env.tau / 2)
    with pytest.raises(ValueError, match="integer multiple"):
        env.vmap_sim_ahead_policy(state, ok, 3, env.tau, env.tau * 1.5)
    # everything in order: what is left is the device, by name (there is no CPU fallback)
    with pytest.raises(RuntimeError, match="vmap_sim_ahead_policy: tensors must live on a HIP device"):
        env.vmap_sim_ahead_policy(state, ok, 3, env.tau, env.tau)
