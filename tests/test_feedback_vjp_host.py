"""Host side of the closed loop's reverse mode (no GPU):
- the float64 torch twin of tests/helpers_feedback_vjp.py gives the closed-loop forward of helpers_feedback.oracle_closed_loop on every
  main case, and its inputs meet the input condition the GPU tests rely on (kink share, clamp activity);
- the built sim_feedback_vjp_kernel instantiations (and the two small kernels next to them) stay within the register / scratch budget;
- excenv_sim_feedback_vjp refuses by code and whole message, before any launch, what it does not do; the workspace and bytes
  functions are the formulas of include/excenv.h / DESIGN.md §4.12;
- the Python methods refuse by name what they do not do, and the default keyword of vmap_sim_ahead_feedback still refuses."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import helpers_feedback as hf
import helpers_feedback_vjp as hv
from exciting_environments_amd import EnvironmentRegistry, _native
from helpers import ANGLE_OBS
from helpers_budget import budget, check_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
MODELS = ["Pendulum", "MassSpringDamper", "CartPole", "Acrobot", "FluidTank", "Pmsm"]
FN = "excenv_sim_feedback_vjp"


# ---- the twin and its inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", hf.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hf.CASES)
def test_twin_forward_is_the_oracles_closed_loop(env_name, deadtime, solver):
    """Within 1e-12 of full scale (the floor tests/test_gpu_feedback.py uses), wrapped angles on the circle"""
    _, _, _, _, out = hv.main_twin(env_name, deadtime, solver)
    want = hf.oracle_case(env_name, deadtime, solver)
    got = out["obs"].detach().numpy()
    d = np.abs(got - want["obs"])
    for c in ANGLE_OBS.get(env_name, []):
        d[..., c] = np.minimum(d[..., c], np.abs(2.0 - d[..., c]))
    dist = float(d.max()) / float(np.max(np.abs(want["obs"])))
    da = float(np.max(np.abs(out["actions"].detach().numpy() - want["actions"])))
    dz = float(np.max(np.abs(out["z"].detach().numpy() - want["z"])))
    print(f"{env_name} deadtime {deadtime} {solver}: observations {dist:.3e}, actions {da:.3e}, z {dz:.3e}")
    assert dist <= 1e-12 and da <= 1e-12 and dz <= 1e-12


@pytest.mark.parametrize("solver", hf.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hf.CASES)
def test_input_condition_of_the_main_cases(env_name, deadtime, solver):
    """On the twin alone: at most KINK_CAP of the environments come within KINK_MARGIN of a kink of the model or a clamp bound of the
    policy; the action clamp is active for 1 % .. 50 % of the entries, the integrator's for at least one."""
    _, _, twin, _, out = hv.main_twin(env_name, deadtime, solver)
    kd = twin.kink_distance().numpy()
    share = float(np.mean(kd < hv.KINK_MARGIN))
    print(f"{env_name} deadtime {deadtime} {solver}: within the margin {share:.4f}, action clamp active {out['clamped']:.3f}, "
          f"integrator clamp active on {out['z_clamped']} entries")
    assert share <= hv.KINK_CAP
    assert 0.01 <= out["clamped"] <= 0.5
    assert out["z_clamped"] >= 1


# ---- the built kernels --------------------------------------------------------------------------------------------------------------
def test_kernels_exist_and_stay_within_the_register_and_scratch_budget():
    """tools/loop_code_size.py on the built library: the 36 instantiations of the reverse kernel (six models x three solvers x two
    element types) are all there, use no scratch memory and at most 256 vector registers (none is pinned to one wave per SIMD);
    the integrator pre-pass and the gain-gradient kernel (six models x two element types each) likewise."""
    res, spans = budget("sim_feedback_vjp_kernel")
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"sim_feedback_vjp_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]}")
    assert len(res) == 36, len(res)
    check_budget(res, spans)
    for name in ("feedback_z_rows_kernel", "feedback_gain_grad_kernel"):
        small, _ = budget(name)
        assert len(small) == 12, (name, len(small))
        over = {k: v for k, v in small.items() if v["scratch"] != 0 or v["vgpr"] > 256}
        assert not over, over


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_sim_feedback_vjp\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_sim_feedback_vjp_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_sim_feedback_vjp_bytes\s*\(", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # additions: a binder probes for the symbols
    lib = ctypes.CDLL(_native.library_path())
    assert all(hasattr(lib, n) for n in (FN, FN + "_workspace_bytes", FN + "_bytes"))
    assert len(_native.PROTOTYPES[FN][1]) == 15 and _native.STRUCTS[_native.FeedbackVjp] == "excenv_feedback_vjp_t"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _record(**kw):
    ptrs = (ctypes.c_void_p * 8)(*([64] * 8))
    r = _native.FeedbackVjp(64, None, 4, -1.0, 1.0, 64, ctypes.addressof(ptrs), 64, None, None, None, None, None, None,
                            ctypes.addressof(ptrs), 64, None, None, 64, None)
    r._keep = ptrs
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(env=0, solver=0, dtype=0, B=4, K=3, sub=1, props=None, control=None, opts=None, rec=None, ws=vp(64), ws_bytes=1 << 40,
          no_props=False, no_rec=False):
    lib = _native.lib()
    p = props if props is not None else _native.Props()
    r = rec if rec is not None else _record()
    rc = lib.excenv_sim_feedback_vjp(env, solver, dtype, i64(B), i64(K), i32(sub), None if no_props else ctypes.byref(p),
                                     None if control is None else ctypes.byref(control), dbl(1e-4), dbl(1e-4),
                                     None if no_rec else ctypes.byref(r), ws, i64(ws_bytes),
                                     None if opts is None else ctypes.byref(opts), None)
    return rc, lib.excenv_last_error().decode()


def test_refusals_come_back_by_code_and_whole_message_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    assert _call(no_props=True) == (ENULL, f"{FN}: props is NULL")
    assert _call(no_rec=True) == (ENULL, f"{FN}: call is NULL")
    table = [
        (dict(gain=None), ENULL, "call->gain is NULL"),
        (dict(state_traj=None), ENULL, "call->state_traj (the reverse pass reads the saved rows) is NULL"),
        (dict(obs_traj=None), ENULL, "call->obs_traj (the gain gradients read the saved observation rows) is NULL"),
        (dict(actions=None), ENULL, "call->actions is NULL"),
        (dict(grad_state0=None), ENULL, "call->grad_state0 is NULL"),
        (dict(grad_ff=None), ENULL, "call->grad_ff (the gain gradients read it) is NULL"),
        (dict(integral_gain=64, grad_z0=64), ENULL, "call->grad_zi (with integral_gain; the gain gradients read it) is NULL"),
        (dict(integral_gain=64, grad_zi=64), ENULL, "call->grad_z0 (with integral_gain) is NULL"),
        (dict(grad_integral_gain=64), ENULL, "call->integral_gain (with grad_integral_gain) is NULL"),
        (dict(gain_batch=3), EINVAL, "call->gain_batch must be 1 (one gain set for all) or the batch size 4 (got 3)"),
        (dict(clip_lo=1.0, clip_hi=-1.0), EINVAL, "call->clip_lo = 1 and call->clip_hi = -1 are not an interval (-inf / +inf: no clamp)"),
        (dict(clip_lo=float("nan")), EINVAL, "call->clip_lo = nan and call->clip_hi = 1 are not an interval (-inf / +inf: no clamp)"),
    ]
    for kw, code, text in table:
        assert _call(rec=_record(**kw)) == (code, f"{FN}: {text}"), kw
    # K == 0 needs neither the actions nor the rows the gain gradients read; B == 0 ends every valid call without a launch
    assert _call(B=0, K=0, rec=_record(actions=None, grad_ff=None, gain_batch=0))[0] == 0
    assert _call(B=0, rec=_record(gain_batch=1))[0] == 0
    # PMSM with substeps != 1, a forced width that cannot be had, a workspace that is too small
    assert _call(env=5, sub=2) == (EINVAL, f"{FN}: PMSM: obs_stepsize must equal action_stepsize (substeps = 2; reference pmsm_env.py:787)")
    for v in (2, 4):
        assert _call(opts=_native.LaunchOpts(v, 0, 0, 0)) == (
            EINVAL, f"{FN}: opts.envs_per_lane = {v} is not available (this kernel has the one-environment-per-lane form only)")
    assert _call(B=0, rec=_record(gain_batch=0), opts=_native.LaunchOpts(1, 0, 0, 0))[0] == 0
    need = _native.lib().excenv_sim_feedback_vjp_workspace_bytes(0, 0, 4, 3, 0, 1, 1)
    rec = _record(gain_batch=1, integral_gain=64, grad_zi=64, grad_z0=64)
    assert need > 0 and _call(rec=rec, ws_bytes=need - 1) == (
        EINVAL, f"{FN}: workspace too small: {need} bytes needed (excenv_sim_feedback_vjp_workspace_bytes), {need - 1} given")
    assert _call(rec=rec, ws=None) == (
        EINVAL, f"{FN}: workspace too small: {need} bytes needed (excenv_sim_feedback_vjp_workspace_bytes), 0 given")
    # the saturated PMSM, per-environment property arrays
    p = _native.Props()
    lut = _native.PmsmLut(4, 4, 64, 64, 64)
    p.pmsm_lut = ctypes.pointer(lut)
    assert _call(env=5, props=p) == (EUNSUPPORTED, f"{FN}: the saturated PMSM (pmsm_lut) has no reverse mode")
    for field in ("static_params", "state_max", "action_min"):
        p = _native.Props()
        getattr(p, field)[0].per_env = 64
        assert _call(props=p) == (EUNSUPPORTED, f"{FN}: per-environment property arrays are not supported (broadcast properties only)"), field
    # bad values; the control record goes through the checks of every other call
    assert _call(env=9)[0] == EINVAL and _call(solver=3)[0] == EINVAL and _call(dtype=2)[0] == EINVAL and _call(B=-1)[0] == EINVAL
    assert _call(K=-1) == (EINVAL, f"{FN}: bad K=-1 or substeps=1") and _call(sub=0) == (EINVAL, f"{FN}: bad K=3 or substeps=0")
    c = _native.Control()
    c.n_control = 1
    assert _call(control=c) == (ENULL, f"{FN}: reference[0] is NULL")
    c.reference[0] = 64
    c.control_idx[0] = 2  # the pendulum has two state leaves
    assert _call(control=c) == (EINVAL, f"{FN}: control_idx[0] out of range")


def test_workspace_and_bytes_functions_are_the_formulas():
    lib = _native.lib()
    up = lambda n: (n + 255) // 256 * 256  # every part of a workspace starts on a 256-byte boundary (sim_plan.hpp align_up)
    for env in range(6):
        S, A, O, _ = _native.env_dims(env)
        for dtype, w in ((_native.F32, 4), (_native.F64, 8)):
            for nc, B, K, integral in itertools.product((0, 2), (1, 326, 70000), (0, 7), (0, 1)):
                OW = O + nc
                for Bg in {1, B}:
                    psum = lib.excenv_param_grad_sum_workspace_bytes(dtype, B, _native.MAX_STATIC)
                    want = (up(w * K * A * B) if integral else 0) + ((up(w * (2 if integral else 1) * A * OW * B) + psum) if Bg == 1 else 0)
                    assert lib.excenv_sim_feedback_vjp_workspace_bytes(env, dtype, B, K, nc, Bg, integral) == want, (env, dtype, nc, B, K, Bg)
                for sub, go, gs, ga in itertools.product((1, 3), (0, 1), (0, 1), (0, 1)):
                    sets = 2 if integral else 1
                    want = w * (sub * (S + go * O + gs * S) + A * (sets + ga) + A * sets + integral * (OW + A) + sets * (OW + A))
                    assert lib.excenv_sim_feedback_vjp_bytes(env, dtype, nc, sub, integral, go, gs, ga) == want
    assert lib.excenv_sim_feedback_vjp_workspace_bytes(17, 0, 4, 3, 0, 1, 0) == -1
    assert lib.excenv_sim_feedback_vjp_workspace_bytes(0, 5, 4, 3, 0, 1, 0) == -1
    assert lib.excenv_sim_feedback_vjp_workspace_bytes(0, 0, 4, 3, 0, 3, 0) == -1
    assert lib.excenv_sim_feedback_vjp_workspace_bytes(0, 0, 4, -1, 0, 1, 0) == -1
    assert lib.excenv_sim_feedback_vjp_bytes(17, 0, 0, 1, 0, 0, 0, 0) == -1 and lib.excenv_sim_feedback_vjp_bytes(0, 0, 0, 0, 0, 0, 0, 0) == -1
    assert lib.excenv_sim_feedback_vjp_bytes(0, 0, 9, 1, 0, 0, 0, 0) == -1


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def test_python_refuses_by_name_what_the_reverse_mode_does_not_do():
    gain = torch.zeros(1, 2)
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    _, state = env.vmap_reset()
    # the default keyword: exactly the refusal of before, its message extended behind the matched text
    env.differentiable = True
    with pytest.raises(ValueError, match="env.differentiable with an input that requires grad.*differentiable=True"):
        env.vmap_sim_ahead_feedback(state, gain.clone().requires_grad_(), 3, env.tau, env.tau)
    env.differentiable = False
    g = gain.clone().requires_grad_()
    env.store_state_trajectory = False
    with pytest.raises(ValueError, match=r"differentiable=True\): store_state_trajectory=False"):
        env.vmap_sim_ahead_feedback(state, g, 3, env.tau, env.tau, differentiable=True)
    env.store_state_trajectory = True
    for layout in ("env_major", "tiled"):
        env.traj_layout = layout
        with pytest.raises(ValueError, match=f"traj_layout='{layout}'"):
            env.vmap_sim_ahead_feedback(state, g, 3, env.tau, env.tau, differentiable=True)
        with pytest.raises(ValueError, match=f"vmap_sim_ahead_feedback_vjp: traj_layout='{layout}'"):
            env.vmap_sim_ahead_feedback_vjp(state, gain, None, None, torch.zeros(4, 3, 1), env.tau, env.tau)
    env.traj_layout = "lane_major"
    env.sim_ahead_semantics = "ahead_accumulated_t"
    with pytest.raises(ValueError, match="ahead_accumulated_t"):
        env.vmap_sim_ahead_feedback(state, g, 3, env.tau, env.tau, differentiable=True)
    with pytest.raises(ValueError, match="vmap_sim_ahead_feedback_vjp: sim_ahead_semantics='ahead_accumulated_t'"):
        env.vmap_sim_ahead_feedback_vjp(state, gain, None, None, torch.zeros(4, 3, 1), env.tau, env.tau)
    env.sim_ahead_semantics = "ahead"
    with pytest.raises(ValueError, match="`states` is None"):
        env.vmap_sim_ahead_feedback_vjp(state, gain, None, None, torch.zeros(4, 3, 1), env.tau, env.tau)
    # per-environment properties, a static parameter that requires grad
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", static_params={"g": torch.full((4,), 9.81), "l": 1.0, "m": 1.0})
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match=r"differentiable=True\): per-environment"):
        env.vmap_sim_ahead_feedback(state, g, 3, env.tau, env.tau, differentiable=True)
    with pytest.raises(ValueError, match="vmap_sim_ahead_feedback_vjp: per-environment"):
        env.vmap_sim_ahead_feedback_vjp(state, gain, None, None, torch.zeros(4, 3, 1), env.tau, env.tau)
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu",
                                            static_params={"g": 9.81, "l": torch.tensor(1.0, requires_grad=True), "m": 1.0})
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match="static parameter 'l' requires grad"):
        env.vmap_sim_ahead_feedback(state, g, 3, env.tau, env.tau, differentiable=True)
    assert env.last_feedback_vjp_launch == "" and env.last_feedback_vjp_cotangents is None


def test_saturated_pmsm_is_refused_by_name():
    from helpers_feedback import saturated_env

    env, _, _, _ = saturated_env(4, torch.float32, "euler", "cpu")
    _, state = env.vmap_reset()
    g = torch.zeros(2, 8, requires_grad=True)
    with pytest.raises(ValueError, match=r"differentiable=True\): the saturated PMSM has no reverse mode"):
        env.vmap_sim_ahead_feedback(state, g, 3, env.tau, env.tau, differentiable=True)
    with pytest.raises(ValueError, match="vmap_sim_ahead_feedback_vjp: the saturated PMSM has no reverse mode"):
        env.vmap_sim_ahead_feedback_vjp(state, g.detach(), None, None, torch.zeros(4, 3, 2), env.tau, env.tau)
