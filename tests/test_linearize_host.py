"""Host side of the batched linearisation (no GPU): the built step_jac_kernel instantiations stay within the register / scratch /
loop budget, excenv_step_jacobian rejects by code and name what it does not do before any launch, excenv_step_jacobian_bytes is the
formula of DESIGN.md §4.10, and the Python methods refuse by name on CPU environments."""
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
    assert re.search(r"\bint\s+excenv_step_jacobian\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_step_jacobian_bytes\s*\(", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # additions: a binder probes for the symbols
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_step_jacobian") and hasattr(lib, "excenv_step_jacobian_bytes")
    assert lib.excenv_abi_version() == 7
    assert len(_native.PROTOTYPES["excenv_step_jacobian"][1]) == 21 and len(_native.PROTOTYPES["excenv_step_jacobian_bytes"][1]) == 3


def test_step_jac_kernels_exist_and_stay_within_the_register_scratch_and_loop_budget():
    """tools/loop_code_size.py on the built library: the 36 instantiations (six models x three solvers x two element types) are all
    there, use no scratch memory and at most 256 vector registers, and their row loop is under 60 KB."""
    res, spans = budget("step_jac_kernel")
    for other in ("step_vjp_kernel", "rew_vjp_kernel", "sim_ahead_vjp_kernel"):  # what the other host tests count kernels by
        assert not [k for k in res if other in k], other
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"step_jac_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]} loop {spans[hit[0]][0]} B of {spans[hit[0]][1]} B")
    assert len(res) == 36, len(res)
    assert 0 < check_budget(res, spans)[1][0]
    assert all(v[0] > 0 for v in spans.values()), "the row loop is a run-time loop in every instantiation"


def _call(env=0, solver=0, dtype=0, B=4, rows=1, substeps=1, props=None, n_control=0, opts=None, null=None, row_kind=0, use_props=True):
    lib = _native.lib()
    p = props if props is not None else _native.Props()
    ptrs = lambda: (ctypes.c_void_p * 8)(*([64] * 8))
    a = dict(state_in=ptrs(), state_out=ptrs(), action=vp(64), jacobian=vp(64))
    if null in a:
        a[null] = None
    elif null is not None:  # "state_out[1]": one entry of a pointer array
        name, j = null[:-3], int(null[-2])
        a[name][j] = None
    rc = lib.excenv_step_jacobian(env, solver, dtype, i64(B), i64(rows), i32(substeps), ctypes.byref(p) if use_props else None,
                                  i32(n_control), dbl(1e-4), dbl(1e-4), a["state_in"], a["state_out"], i64(B), a["action"], i64(0),
                                  i64(1), i64(1), row_kind, a["jacobian"], None if opts is None else ctypes.byref(opts), None)
    return rc, lib.excenv_last_error()


def test_validation_errors_come_back_by_code_and_name_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    for name in ("state_in", "state_out", "action", "jacobian"):
        rc, msg = _call(null=name)
        assert rc == ENULL and name.encode() in msg, (name, rc, msg)
    for name, word in (("state_in[1]", b"state_in pointer 1"), ("state_out[0]", b"state_out pointer 0")):
        rc, msg = _call(null=name)
        assert rc == ENULL and word in msg, (name, rc, msg)
    rc, msg = _call(use_props=False)
    assert rc == ENULL and b"props" in msg
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
    # PMSM: one solver step per action row (the existing rule)
    rc, msg = _call(env=5, substeps=2, rows=4)
    assert rc == EUNSUPPORTED and b"PMSM" in msg and b"obs_stepsize" in msg
    # bad values
    assert _call(env=9)[0] == EINVAL and _call(env=-1)[0] == EINVAL and _call(solver=3)[0] == EINVAL and _call(dtype=2)[0] == EINVAL
    rc, msg = _call(B=-1)
    assert rc == EINVAL and b"batch size" in msg
    rc, msg = _call(rows=-1)
    assert rc == EINVAL and b"rows" in msg
    for s in (0, -3):
        rc, msg = _call(substeps=s)
        assert rc == EINVAL and b"substeps" in msg
    rc, msg = _call(row_kind=2)
    assert rc == EINVAL and b"row_kind" in msg
    rc, msg = _call(n_control=-1)
    assert rc == EINVAL and b"n_control" in msg
    # a forced width that cannot be had: only one step instance per lane is built
    for dtype, v in ((0, 4), (1, 2), (0, 2)):
        rc, msg = _call(dtype=dtype, opts=_native.LaunchOpts(v, 0, 0, 0))
        assert rc == EINVAL and b"envs_per_lane" in msg
    assert _call(B=0, opts=_native.LaunchOpts(1, 0, 0, 0))[0] == 0
    # B == 0 or rows == 0: nothing to do, whatever the arrays' addresses are
    assert _call(B=0, null="action")[0] == 0 and _call(rows=0, null="jacobian")[0] == 0 and _call(B=0, rows=0, null="state_in")[0] == 0


def test_step_jacobian_bytes_is_the_formula():
    lib = _native.lib()
    for env in range(6):
        S, A, O, _ = _native.env_dims(env)
        for dtype, w in ((_native.F32, 4), (_native.F64, 8)):
            for kind, R in ((_native.JAC_STATE, S), (_native.JAC_OBS, O)):
                assert lib.excenv_step_jacobian_bytes(env, dtype, kind) == w * (2 * S + A + R * (S + A)), (env, dtype, kind)
    assert lib.excenv_step_jacobian_bytes(17, 0, 0) == -1 and lib.excenv_step_jacobian_bytes(0, 5, 0) == -1
    assert lib.excenv_step_jacobian_bytes(0, 0, 2) == -1
    assert _native.step_jacobian_bytes(5, torch.float32, "state") == 4 * (2 * 7 + 2 + 7 * 9)
    assert _native.step_jacobian_bytes(5, torch.float64, "obs") == 8 * (2 * 7 + 2 + 8 * 9)


def test_python_refuses_by_name_what_a_linearisation_does_not_do():
    """Raised before anything touches the device: these environments live on the CPU, where no kernel can run."""
    from conftest import GOLDEN
    from exciting_environments_amd import MotorVariant

    # per-environment property arrays
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", static_params={"g": torch.full((4,), 9.81), "l": 1.0, "m": 1.0})
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match="per-environment"):
        env.vmap_linearize(state, torch.zeros(4, 1))
    with pytest.raises(ValueError, match="per-environment"):
        env.vmap_linearize(state, torch.zeros(4, 1), state, rows="obs")
    env.sim_ahead_semantics = "step"
    with pytest.raises(ValueError, match="per-environment"):
        env.vmap_linearize_ahead(state, torch.zeros(4, 3, 1), env.tau, env.tau)
    # the saturated PMSM
    env = EnvironmentRegistry.PMSM.make(batch_size=4, saturated=True, motor_variant=MotorVariant.BRUSA, device="cpu",
                                        pmsm_lut_path=os.path.join(GOLDEN, "pmsm"))
    _, state = env.vmap_reset()
    with pytest.raises(ValueError, match="saturated"):
        env.vmap_linearize(state, torch.zeros(4, 2))
    env.sim_ahead_semantics = "step"
    with pytest.raises(ValueError, match="saturated"):
        env.vmap_linearize_ahead(state, torch.zeros(4, 3, 2), env.tau, env.tau)
    # the semantics whose carried state is not the saved row, by name and with the reason
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    _, state = env.vmap_reset()
    assert env.sim_ahead_semantics == "ahead"
    with pytest.raises(ValueError, match=r"'ahead'.*carried state.*not the saved row"):
        env.vmap_linearize_ahead(state, torch.zeros(4, 3, 1), env.tau, env.tau)
    env.sim_ahead_semantics = "ahead_accumulated_t"
    with pytest.raises(ValueError, match=r"'ahead_accumulated_t'.*carried state.*not the saved row"):
        env.vmap_linearize_ahead(state, torch.zeros(4, 3, 1), env.tau, env.tau)
    # the forward-only layouts, by name
    env.sim_ahead_semantics = "step"
    for layout in ("env_major", "tiled"):
        env.traj_layout = layout
        with pytest.raises(ValueError, match=layout):
            env.vmap_linearize_ahead(state, torch.zeros(4, 3, 1), env.tau, env.tau)
    env.traj_layout = "lane_major"
    with pytest.raises(ValueError, match="rows must be"):
        env.vmap_linearize(state, torch.zeros(4, 1), state, rows="reward")
    assert env.last_linearize_launch == ""


def test_the_fp32_inputs_keep_the_excluded_share_under_the_cap():
    """tests/test_gpu_linearize.py compares fp32 Jacobians on the environments the twin sees at least KINK_MARGIN from a kink: on
    its inputs (helpers_step_vjp.step_inputs, fp32-representable values, every model and solver) at most KINK_CAP of them are left out."""
    from helpers_step_vjp import check_fp32_excluded_share

    check_fp32_excluded_share()
