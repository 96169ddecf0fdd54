"""Host side of the closed-loop trajectories (no GPU): the header declares excenv_sim_feedback and _native mirrors it, the entry point
refuses by code and whole message what it does not do before any launch, every built sim_feedback_kernel instantiation is free of
scratch memory, the test inputs clamp some but not most actions on the float64 oracle loop, and `vmap_sim_ahead_feedback` raises the
named exceptions on CPU environments."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget
import helpers_feedback as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
MODELS = ["Pendulum", "MassSpringDamper", "CartPole", "Acrobot", "FluidTank", "Pmsm", "PmsmSat"]
INF = math.inf


def test_header_declares_native_mirrors_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_sim_feedback\s*\(", hdr)
    assert re.search(r"\}\s*excenv_feedback_t\s*;", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # an addition: a binder probes for the symbol
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_sim_feedback")
    assert lib.excenv_abi_version() == 7 and _native.ABI_VERSION == 7
    assert len(_native.PROTOTYPES["excenv_sim_feedback"][1]) == 18
    assert _native.STRUCTS[_native.Feedback] == "excenv_feedback_t"
    assert [f[0] for f in _native.Feedback._fields_] == ["gain", "integral_gain", "gain_batch", "feedforward", "z_in", "z_out", "clip_lo",
                                                         "clip_hi"]


# ---- refusals: fake 16-byte aligned addresses everywhere, nothing may reach a launch ----------------------------------------------
def _call(env=0, B=4, K=2, substeps=1, policy="default", null=None, epl=0, lut=False, **pol):
    """One excenv_sim_feedback call. null: the argument (or policy field) passed as NULL; pol: policy fields to override."""
    lib = _native.lib()
    props = _native.Props()
    keep = []
    if lut:
        keep.append(_native.PmsmLut(4, 4, 64, 64, 64))
        props.pmsm_lut = ctypes.pointer(keep[0])
    ptrs = lambda: (ctypes.c_void_p * 8)(*([64] * 8))
    a = dict(state_in=ptrs(), obs_traj=vp(64), state_traj=ptrs(), last_state=ptrs(), actions_out=vp(64))
    f = dict(gain=64, integral_gain=None, gain_batch=1, feedforward=None, z_in=None, z_out=None, clip_lo=-1.0, clip_hi=1.0)
    f.update(pol)
    if null in a:
        a[null] = None
    elif null in f:
        f[null] = None
    elif null is not None:  # "last_state[1]": one entry of a pointer array
        name, j = null[:-3], int(null[-2])
        a[name][j] = None
    p = _native.Feedback(f["gain"], f["integral_gain"], f["gain_batch"], f["feedforward"], f["z_in"], f["z_out"], f["clip_lo"], f["clip_hi"])
    opts = _native.LaunchOpts(epl, 0, 0, 0)
    rc = lib.excenv_sim_feedback(env, 0, 0, i64(B), i64(K), i32(substeps), ctypes.byref(props), None, dbl(1e-4), dbl(1e-4), a["state_in"],
                                 None if policy is None else ctypes.byref(p), a["obs_traj"], a["state_traj"], a["last_state"],
                                 a["actions_out"], ctypes.byref(opts), None)
    return rc, lib.excenv_last_error().decode()


# what the call is made with, return code, the whole message
REFUSALS = [
    (dict(policy=None), ENULL, "excenv_sim_feedback: policy is NULL"),
    (dict(null="gain"), ENULL, "excenv_sim_feedback: policy->gain is NULL"),
    (dict(null="obs_traj"), ENULL, "excenv_sim_feedback: obs_traj is NULL"),
    (dict(null="last_state"), ENULL, "excenv_sim_feedback: last_state is NULL"),
    (dict(null="state_in"), ENULL, "excenv_sim_feedback: state_in is NULL"),
    (dict(gain_batch=2), EINVAL, "excenv_sim_feedback: policy->gain_batch must be 1 (one gain set for all) or the batch size 4 (got 2)"),
    (dict(gain_batch=0), EINVAL, "excenv_sim_feedback: policy->gain_batch must be 1 (one gain set for all) or the batch size 4 (got 0)"),
    (dict(clip_lo=0.5, clip_hi=0.25), EINVAL,
     "excenv_sim_feedback: policy->clip_lo = 0.5 and policy->clip_hi = 0.25 are not an interval (-inf / +inf: no clamp)"),
    (dict(clip_lo=math.nan), EINVAL,
     "excenv_sim_feedback: policy->clip_lo = nan and policy->clip_hi = 1 are not an interval (-inf / +inf: no clamp)"),
    (dict(clip_hi=math.nan), EINVAL,
     "excenv_sim_feedback: policy->clip_lo = -1 and policy->clip_hi = nan are not an interval (-inf / +inf: no clamp)"),
    (dict(env=5, substeps=2), EINVAL,
     "excenv_sim_feedback: PMSM: obs_stepsize must equal action_stepsize (substeps = 2; reference pmsm_env.py:787)"),
    (dict(env=5, substeps=3, lut=True), EINVAL,
     "excenv_sim_feedback: PMSM: obs_stepsize must equal action_stepsize (substeps = 3; reference pmsm_env.py:787)"),
    (dict(integral_gain=64), ENULL,
     "excenv_sim_feedback: policy->integral_gain without policy->z_out (the integrator state has to go somewhere)"),
    (dict(epl=2), EINVAL,
     "excenv_sim_feedback: opts.envs_per_lane = 2 is not available (this kernel has the one-environment-per-lane form only)"),
    (dict(epl=4), EINVAL,
     "excenv_sim_feedback: opts.envs_per_lane = 4 is not available (this kernel has the one-environment-per-lane form only)"),
    (dict(epl=3), EINVAL, "excenv_sim_feedback: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)"),
    (dict(null="last_state[1]"), ENULL, "excenv_sim_feedback: state pointer 1 is NULL"),
    (dict(null="state_traj[0]"), ENULL, "excenv_sim_feedback: state_traj pointer 0 is NULL"),
    (dict(K=-1), EINVAL, "excenv_sim_feedback: bad K=-1 or substeps=1"),
    (dict(substeps=0), EINVAL, "excenv_sim_feedback: bad K=2 or substeps=0"),
    (dict(B=-1), EINVAL, "excenv_sim_feedback: bad batch size -1"),
    (dict(env=7), EINVAL, "excenv_sim_feedback: bad env id 7"),
    (dict(env=0, lut=True), EINVAL, "pmsm_lut is only valid for EXCENV_PMSM"),
]


@pytest.mark.parametrize("how,rc,message", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in REFUSALS])
def test_the_refusal_comes_back_by_code_and_whole_message(how, rc, message):
    assert _call(**how) == (rc, message)


def test_an_empty_batch_is_ok_without_a_launch():
    """B == 0: nothing to do — and no GPU here, so a launch would have come back as EXCENV_EHIP. (K == 0 launches: row 0 only; the
    GPU suite covers it.)"""
    assert _call(B=0)[0] == 0
    assert _call(B=0, K=0, gain_batch=0)[0] == 0  # gain_batch == B
    assert _call(B=0, epl=1)[0] == 0


def test_sim_feedback_kernels_exist_and_use_no_scratch():
    """tools/loop_code_size.py kernel_resources on the built library: the 42 instantiations (seven models, the saturated PMSM
    included, x three solvers x two element types) are all there and none has a private segment."""
    res, spans = budget("sim_feedback_kernel")
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"sim_feedback_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]} loop {spans[hit[0]][0]} B of {spans[hit[0]][1]} B")
    assert len(res) == 42, len(res)
    assert all(v["scratch"] == 0 for v in res.values()), {k: v for k, v in res.items() if v["scratch"]}
    assert max(v[0] for v in spans.values()) < 60 * 1024  # the trajectory loop stays inside the instruction cache


# ---- the input condition: neither "never clamps" nor "always clamps" can hide a fault ---------------------------------------------
@pytest.mark.parametrize("solver", hf.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hf.CASES)
def test_the_inputs_clamp_some_but_not_most_actions_on_the_oracle(env_name, deadtime, solver):
    r = hf.oracle_case(env_name, deadtime, solver)
    print(f"{env_name} deadtime {deadtime} {solver}: clamped share {r['clamped']:.3f}, integrator at its clamp "
          f"{float(np.mean(np.abs(r['z']) >= 1.0)):.3f}")
    assert 0.02 <= r["clamped"] <= 0.60
    assert np.all(np.isfinite(r["obs"])) and r["obs"].shape == (hf.B_MAIN, hf.K_MAIN * hf.substeps_of(env_name) + 1, hf.obs_width(env_name))
    assert 0.0 < float(np.mean(np.abs(r["z"]) >= 1.0)) < 0.9  # the anti-windup clamp is reached by some integrators, not by all


def test_the_saturated_inputs_clamp_some_but_not_most_actions_on_the_oracle():
    env, props, keep, spec = hf.saturated_env(hf.B_MAIN, torch.float64, "euler", "cpu")
    inp = hf.feedback_inputs("pmsm", spec)
    r = hf.oracle_closed_loop("pmsm", "euler", props, inp, spec["tau"])
    print(f"saturated PMSM: clamped share {r['clamped']:.3f}")
    assert 0.02 <= r["clamped"] <= 0.60 and np.all(np.isfinite(r["obs"]))


def test_policy_restatement_is_the_written_contract():
    """policy_np against the formula spelled out entry by entry (one environment, two action components, three columns)"""
    ob = np.array([[0.5, -0.25, 0.125]])
    g = np.array([[1.0, 2.0, 4.0], [-8.0, 0.5, 0.25]])
    h = np.array([[100.0, 0.0, 0.0], [0.0, 0.0, -800.0]])
    a, z, raw, mag, zmag = hf.policy_np(ob, g, h, np.array([[0.25, -0.5]]), np.array([[0.125, 0.25]]), (-1.0, 1.0), 1e-2)
    assert raw.tolist() == [[0.25 + 0.125 + 0.5 - 0.5 + 0.5, -0.5 + 0.25 - 4.0 - 0.125 + 0.03125]]
    assert a.tolist() == [[0.875, -1.0]]
    assert z.tolist() == [[0.125 + 1e-2 * 50.0, max(0.25 + 1e-2 * -100.0, -1.0)]]
    assert mag.tolist() == [[0.25 + 0.125 + 1.5, 0.5 + 0.25 + 4.0 + 0.125 + 0.03125]]
    a, z, raw, _, _ = hf.policy_np(ob, g, None, None, None, None, 1e-2)
    assert z is None and a.tolist() == raw.tolist() == [[0.5, -4.0 - 0.125 + 0.03125]]


# ---- Python argument faults (CPU environments: raised before anything touches a device) ---------------------------------------------
def _cpu_env(**kw):
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", **kw)
    _, state = env.vmap_reset()
    return env, state


def test_python_refuses_by_name_what_a_closed_loop_does_not_do():
    env, state = _cpu_env()
    gain = torch.zeros(1, 2)
    for layout in ("env_major", "tiled"):
        env.traj_layout = layout
        with pytest.raises(ValueError, match=f"vmap_sim_ahead_feedback: traj_layout='{layout}'"):
            env.vmap_sim_ahead_feedback(state, gain, 3, env.tau, env.tau)
    env.traj_layout = "lane_major"
    env.sim_ahead_semantics = "ahead_accumulated_t"
    with pytest.raises(ValueError, match="sim_ahead_semantics='ahead_accumulated_t'"):
        env.vmap_sim_ahead_feedback(state, gain, 3, env.tau, env.tau)
    env.sim_ahead_semantics = "ahead"
    env.differentiable = True
    for kw in (dict(gain=gain.clone().requires_grad_()), dict(gain=gain, feedforward=torch.zeros(4, 3, 1, requires_grad=True)),
               dict(gain=gain, integral_gain=gain.clone().requires_grad_()),
               dict(gain=gain, integral_gain=gain, integrator_state=torch.zeros(4, 1, requires_grad=True))):
        with pytest.raises(ValueError, match="env.differentiable with an input that requires grad"):
            env.vmap_sim_ahead_feedback(state, kw.pop("gain"), 3, env.tau, env.tau, **kw)
    state.physical_state.theta = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError, match="env.differentiable with an input that requires grad"):
        env.vmap_sim_ahead_feedback(state, gain, 3, env.tau, env.tau)
    assert env.last_feedback_launch == ""


def test_python_shape_faults_are_assertion_errors_with_a_message():
    env, state = _cpu_env()
    ok = torch.zeros(1, 2)
    with pytest.raises(AssertionError, match=r"The gain needs to be of shape .*\(1, 2\) or \(4, 1, 2\), but \(2, 1\)"):
        env.vmap_sim_ahead_feedback(state, torch.zeros(2, 1), 3, env.tau, env.tau)
    with pytest.raises(AssertionError, match=r"The integral gain needs to be of shape"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau, integral_gain=torch.zeros(3, 1, 2))
    with pytest.raises(AssertionError, match="The feedforward needs to have three dimensions"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau, feedforward=torch.zeros(4, 3))
    with pytest.raises(AssertionError, match="n_actions is 5, but the feedforward has 3 action rows"):
        env.vmap_sim_ahead_feedback(state, ok, 5, env.tau, env.tau, feedforward=torch.zeros(4, 3, 1))
    with pytest.raises(AssertionError, match="n_actions is needed"):
        env.vmap_sim_ahead_feedback(state, ok, None, env.tau, env.tau)
    with pytest.raises(AssertionError, match="The integrator state needs to be of shape"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau, integral_gain=ok, integrator_state=torch.zeros(4))
    with pytest.raises(AssertionError, match="integrator_state without integral_gain"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau, integrator_state=torch.zeros(4, 1))
    with pytest.raises(AssertionError, match="clip needs to be"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau, clip=(1.0, -1.0))
    with pytest.raises(AssertionError, match="action stepsize should be greater or equal"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau / 2)
    with pytest.raises(ValueError, match="integer multiple"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau * 1.5)
    # everything in order: what is left is the device, by name (there is no CPU fallback)
    with pytest.raises(RuntimeError, match="vmap_sim_ahead_feedback: tensors must live on a HIP device"):
        env.vmap_sim_ahead_feedback(state, ok, 3, env.tau, env.tau)
