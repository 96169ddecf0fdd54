"""Host side of the reverse-mode step (no GPU): the built step_vjp_kernel instantiations stay within the register / scratch / loop
budget, excenv_step_vjp rejects by code and name what it does not do before any launch, and excenv_step_vjp_bytes is the formula of
DESIGN.md §4.9 "Step"."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget, check_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
MODELS = ["Pendulum", "MassSpringDamper", "CartPole", "Acrobot", "FluidTank", "Pmsm"]


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_step_vjp\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_step_vjp_bytes\s*\(", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # additions: a binder probes for the symbols
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_step_vjp") and hasattr(lib, "excenv_step_vjp_bytes")
    assert len(_native.PROTOTYPES["excenv_step_vjp"][1]) == 17 and len(_native.PROTOTYPES["excenv_step_vjp_bytes"][1]) == 6


def test_step_vjp_kernels_exist_and_stay_within_the_register_scratch_and_loop_budget():
    """tools/loop_code_size.py on the built library: the 36 instantiations (six models x three solvers x two element types, one
    environment per lane) are all there, use no scratch memory and at most 256 vector registers, and have no loop of 60 KB."""
    res, spans = budget("step_vjp_kernel")
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"step_vjp_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}ELi1EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]}")
    assert len(res) == 36, len(res)
    check_budget(res, spans)


def _call(env=0, solver=0, dtype=0, B=4, props=None, control=None, opts=None, grad_reward=None, null=None, grad_obs=64):
    lib = _native.lib()
    p = props if props is not None else _native.Props()
    ptrs = lambda: (ctypes.c_void_p * 8)(*([64] * 8))
    a = dict(state_in=ptrs(), action=vp(64), state_out=ptrs(), grad_state_in=ptrs(), grad_action=vp(64))
    if null in a:
        a[null] = None
    elif null is not None:  # "state_out[1]": one entry of a pointer array
        name, j = null[:-3], int(null[-2])
        a[name][j] = None
    rc = lib.excenv_step_vjp(env, solver, dtype, i64(B), ctypes.byref(p), None if control is None else ctypes.byref(control), dbl(1e-4),
                             a["state_in"], a["action"], a["state_out"], vp(grad_obs), ptrs(), grad_reward, a["grad_state_in"],
                             a["grad_action"], None if opts is None else ctypes.byref(opts), None)
    return rc, lib.excenv_last_error()


def test_validation_errors_come_back_by_code_and_name_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    # a NULL required pointer, named
    for name in ("state_in", "action", "state_out", "grad_state_in", "grad_action"):
        rc, msg = _call(null=name)
        assert rc == ENULL and name.encode() in msg, (name, rc, msg)
    for name, word in (("state_in[1]", b"state_in pointer 1"), ("state_out[0]", b"state_out pointer 0"),
                       ("grad_state_in[1]", b"grad_state_in pointer 1")):
        rc, msg = _call(null=name)
        assert rc == ENULL and word in msg, (name, rc, msg)
    lib = _native.lib()
    one = (ctypes.c_void_p * 8)(*([64] * 8))
    rc = lib.excenv_step_vjp(0, 0, 0, i64(4), None, None, dbl(1e-4), one, vp(64), one, None, None, None, one, vp(64), None, None)
    assert rc == ENULL and b"props" in lib.excenv_last_error()
    # the saturated PMSM
    p = _native.Props()
    lut = _native.PmsmLut(4, 4, 64, 64, 64)
    p.pmsm_lut = ctypes.pointer(lut)
    rc, msg = _call(env=5, props=p)
    assert rc == EUNSUPPORTED and b"saturated" in msg
    # per-environment property arrays: a static parameter, a state bound, an action bound
    for field in ("static_params", "state_max", "action_min"):
        p = _native.Props()
        getattr(p, field)[0].per_env = 64
        rc, msg = _call(props=p)
        assert rc == EUNSUPPORTED and b"per-environment" in msg, field
    # a reward cotangent without control references: no control at all, n_control == 0, a NULL reference
    rc, msg = _call(grad_reward=vp(64))
    assert rc == EUNSUPPORTED and b"grad_reward" in msg and b"control" in msg
    rc, msg = _call(grad_reward=vp(64), control=_native.Control())
    assert rc == EUNSUPPORTED and b"grad_reward" in msg
    c = _native.Control()
    c.n_control = 1
    rc, msg = _call(grad_reward=vp(64), control=c)
    assert rc == ENULL and b"reference[0]" in msg
    c.reference[0] = 64
    c.control_idx[0] = 2  # the pendulum has two state leaves
    rc, msg = _call(grad_reward=vp(64), control=c)
    assert rc == EINVAL and b"control_idx[0]" in msg
    # without a reward cotangent only n_control is read: NULL references are fine there (B == 0 ends the call without a launch)
    c = _native.Control()
    c.n_control = 1
    assert _call(B=0, control=c)[0] == 0
    # a forced width that cannot be had: only one environment per lane is built
    for dtype, v in ((0, 4), (1, 2), (0, 2)):
        rc, msg = _call(dtype=dtype, opts=_native.LaunchOpts(v, 0, 0, 0))
        assert rc == EINVAL and b"envs_per_lane" in msg
    assert _call(B=0, opts=_native.LaunchOpts(1, 0, 0, 0))[0] == 0
    # bad values, misaligned rows
    assert _call(env=9)[0] == EINVAL and _call(solver=3)[0] == EINVAL and _call(dtype=2)[0] == EINVAL and _call(B=-1)[0] == EINVAL
    rc, msg = _call(grad_obs=68)
    assert rc == EINVAL and b"16-byte" in msg
    # B == 0: nothing to do, whatever the arrays' addresses are
    assert _call(B=0, null="action")[0] == 0


def test_step_vjp_bytes_is_the_formula():
    lib = _native.lib()
    for env, reg in enumerate(list(EnvironmentRegistry)[:6]):
        S, A, O, _ = _native.env_dims(env)
        for dtype, w in ((_native.F32, 4), (_native.F64, 8)):
            for nc in (0, 1, 3):
                for go, gs, gr in itertools.product((0, 1), repeat=3):
                    want = w * (2 * S + A) + (w * (O + nc) if go else 0) + (w * S if gs else 0) + (w * (1 + nc) if gr else 0) + w * (S + A)
                    assert lib.excenv_step_vjp_bytes(env, dtype, nc, go, gs, gr) == want, (env, dtype, nc, go, gs, gr)
    assert lib.excenv_step_vjp_bytes(17, 0, 0, 1, 1, 0) == -1 and lib.excenv_step_vjp_bytes(0, 5, 0, 1, 1, 0) == -1
    assert lib.excenv_step_vjp_bytes(0, 0, -1, 1, 1, 0) == -1
    assert _native.step_vjp_bytes(5, torch.float32, 2, True, True, True) == 4 * (2 * 7 + 2) + 4 * 10 + 4 * 7 + 4 * 3 + 4 * 9


def test_python_refuses_by_name_what_a_differentiable_step_does_not_do():
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", static_params={"g": torch.full((4,), 9.81), "l": 1.0, "m": 1.0})
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match="per-environment"):
        env.vmap_step_vjp(state, torch.zeros(4, 1), state)
    env.differentiable = True
    with pytest.raises(ValueError, match="per-environment"):
        env.vmap_step(state, torch.zeros(4, 1, requires_grad=True))
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu",
                                            static_params={"g": 9.81, "l": torch.tensor(1.0, requires_grad=True), "m": 1.0})
    env.differentiable = True
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match="static parameter 'l'"):
        env.vmap_gym_step(state, torch.zeros(4, 1, requires_grad=True))


def test_the_fp32_inputs_keep_the_excluded_share_under_the_cap():
    """tests/test_gpu_step_vjp.py compares fp32 gradients on the environments the twin sees at least KINK_MARGIN from a kink: on
    its inputs (fp32-representable values, every model and solver) at most KINK_CAP of them are left out."""
    from helpers_step_vjp import check_fp32_excluded_share

    check_fp32_excluded_share()
