"""Host side of the reward's reverse mode (no GPU): the C ABI declares and exports excenv_rew_vjp / excenv_rew_reads, the reads
table, rejections before any launch, the CPU `vmap_reward_vjp` (torch autograd over the torch mirror) against central differences of
the fp64 oracle on the very inputs the GPU tests use (tests/helpers_reward_vjp.py: the exclusion cap and the branch coverage are
asserted here on those arrays), and the built rew_vjp_kernel instantiations use no scratch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle
from conftest import ENV_NAMES
from exciting_environments_amd import _native
from helpers import make_env
from helpers_budget import budget
from helpers_reward_vjp import (NARROW_B, ROWS, check_coverage_and_cap, control_sets, expected_reads, make_states, oracle_grads,
                                rel_dist, reward_inputs, tensor, to_np, wide_b)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
EINVAL, ENULL = -1, -2


# ---------------------------------------------------------------------------------------------------------------- 1
def test_header_declares_and_library_exports_the_reward_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_rew_vjp\s*\(", hdr)
    assert re.search(r"\bint\s+excenv_rew_reads\s*\(", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # additions: a binder probes for the symbols
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_rew_vjp") and hasattr(lib, "excenv_rew_reads")
    assert _native.lib().excenv_abi_version() == 7 and _native.ABI_VERSION == 7
    assert len(_native.PROTOTYPES["excenv_rew_vjp"][1]) == 16 and len(_native.PROTOTYPES["excenv_rew_reads"][1]) == 4
    # the pinned prototypes keep their lengths
    assert len(_native.PROTOTYPES["excenv_sim_ahead_vjp"][1]) == 23
    assert len(_native.PROTOTYPES["excenv_sim_ahead_vjp_params"][1]) == 24
    assert len(_native.PROTOTYPES["excenv_rew_trunc_term"][1]) == 15


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_rew_reads_table(env_name):
    fields = oracle.STATE_FIELDS[env_name]
    env_id = oracle.ENV_IDS[env_name]
    sets = control_sets(env_name)
    assert () in sets and all((f,) in sets for f in fields)
    if env_name == "pmsm":
        assert {("i_d",), ("i_d", "i_q"), ("torque",), ("i_d", "i_q", "torque")} <= set(sets)
    elif len(fields) > 1:
        assert any(len(s) > 1 for s in sets)
    for control in sets:
        got = _native.rew_reads(env_id, [fields.index(n) for n in control])
        assert len(got) == _native.MAX_STATE
        assert got[:len(fields)] == expected_reads(env_name, control), control
        assert not any(got[len(fields):])
    if env_name == "pmsm":  # spelled out: the current term needs both currents, the torque term reads the currents too
        idx = lambda *names: [fields.index(n) for n in names]
        assert _native.rew_reads(5, idx("i_d")) == [False] * 8
        assert _native.rew_reads(5, idx("i_d", "i_q")) == [False, False, False, True, True, False, False, False]
        assert _native.rew_reads(5, idx("torque")) == [False, False, False, True, True, True, False, False]
        assert _native.rew_reads(5, idx("i_d", "i_q", "torque")) == [False, False, False, True, True, True, False, False]
    lib = _native.lib()
    out = (ctypes.c_uint8 * 8)()
    assert lib.excenv_rew_reads(9, 0, None, out) == EINVAL
    assert lib.excenv_rew_reads(env_id, 1, (ctypes.c_int32 * 1)(len(fields)), out) == EINVAL and b"control_idx[0]" in lib.excenv_last_error()
    assert lib.excenv_rew_reads(env_id, 0, None, None) == ENULL


# ---------------------------------------------------------------------------------------------------------------- 3
def _call(env=0, dtype=0, B=4, rows=3, props=True, control_idx=(0,), refs=True, state=True, grad=True, outs=(64, 64, 64, 64, 64, 64, 64, 64),
          opts=None, strides=(1, 4), g_strides=(1, 4), ref_strides=None):
    """excenv_rew_vjp on fake pointers: whatever reached a launch would fail differently (EXCENV_EHIP) or crash"""
    lib = _native.lib()
    p = _native.Props()
    c = None
    if control_idx is not None:
        c = _native.Control()
        c.n_control = len(control_idx)
        for j, f in enumerate(control_idx):
            c.control_idx[j] = f
            c.reference[j] = 64 if refs else None
    st = (ctypes.c_void_p * 8)(*([64] * 8)) if state else None
    out = None if outs is None else (ctypes.c_void_p * 8)(*outs)
    rs = None if ref_strides is None else (ctypes.c_int64 * len(ref_strides))(*ref_strides)
    rc = lib.excenv_rew_vjp(env, dtype, i64(B), i64(rows), ctypes.byref(p) if props else None, None if c is None else ctypes.byref(c),
                            rs, st, i64(strides[0]), i64(strides[1]), vp(64) if grad else None, i64(g_strides[0]), i64(g_strides[1]),
                            out, None if opts is None else ctypes.byref(opts), None)
    return rc, lib.excenv_last_error()


def test_rejections_happen_before_any_launch():
    # NULL arguments
    for kw in (dict(props=False), dict(state=False), dict(grad=False), dict(outs=None)):
        rc, msg = _call(**kw)
        assert rc == ENULL and b"NULL" in msg, kw
    rc, msg = _call(refs=False)
    assert rc == ENULL and b"reference[0]" in msg
    # rows = 0, bad ids, a bad control index
    rc, msg = _call(rows=0)
    assert rc == EINVAL and b"rows" in msg
    assert _call(env=9)[0] == EINVAL and _call(dtype=3)[0] == EINVAL and _call(B=-1)[0] == EINVAL
    rc, msg = _call(control_idx=(2,))  # the pendulum has two state fields
    assert rc == EINVAL and b"control_idx[0]" in msg
    # a NULL output for a read leaf names the leaf; one for a leaf that is not read is fine (checked before the launch it never reaches)
    rc, msg = _call(env=2, control_idx=(0, 2), outs=(64, 64, None, 64, 64, 64, 64, 64))
    assert rc == ENULL and b"grad_state_traj pointer 2" in msg
    rc, msg = _call(env=5, control_idx=(5,), outs=(None, None, None, 64, None, 64, None, None))  # torque control reads i_q too
    assert rc == ENULL and b"grad_state_traj pointer 4" in msg
    # a forced width that cannot be had
    rc, msg = _call(opts=_native.LaunchOpts(2, 0, 0, 0))  # fp32: the forms are 1 and 4 environments per lane
    assert rc == EINVAL and b"envs_per_lane = 2" in msg
    rc, msg = _call(dtype=1, opts=_native.LaunchOpts(4, 0, 0, 0))  # fp64: 1 and 2
    assert rc == EINVAL and b"envs_per_lane = 4" in msg
    rc, msg = _call(B=6, strides=(1, 6), g_strides=(1, 6), opts=_native.LaunchOpts(4, 0, 0, 0))  # 6 % 4 != 0
    assert rc == EINVAL and b"envs_per_lane = 4" in msg
    rc, msg = _call(strides=(3, 1), opts=_native.LaunchOpts(4, 0, 0, 0))  # row-major state leaves
    assert rc == EINVAL and b"envs_per_lane = 4" in msg
    rc, msg = _call(ref_strides=(3, 1), opts=_native.LaunchOpts(4, 0, 0, 0))  # a row-major reference
    assert rc == EINVAL and b"envs_per_lane" in msg
    rc, msg = _call(g_strides=(2, 1), opts=_native.LaunchOpts(4, 0, 0, 0))  # a row-major reward cotangent
    assert rc == EINVAL and b"envs_per_lane" in msg
    rc, msg = _call(outs=(72, 64, 64, 64, 64, 64, 64, 64), opts=_native.LaunchOpts(4, 0, 0, 0))  # an output that is not 16-byte aligned
    assert rc == EINVAL and b"envs_per_lane" in msg
    # an empty batch is no error and no launch either
    assert _call(B=0)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- 4
SHAPES = [("wide32", wide_b(4), 4), ("wide64", wide_b(8), 8), ("narrow", NARROW_B, 8), ("narrow32", NARROW_B, 4)]


@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_cpu_reward_vjp_matches_oracle_differences_on_the_gpu_tests_inputs(env_name):
    """torch autograd over the torch mirror (fp64, CPU) within 1e-7 of each leaf's largest magnitude of the oracle's central
    differences; the same loop asserts, on every array the GPU tests use, the exclusion cap and the branch coverage."""
    fields = oracle.STATE_FIELDS[env_name]
    worst = 0.0
    for control in control_sets(env_name):
        for tag, B, elem in SHAPES:
            data = reward_inputs(env_name, control, B, ROWS, elem)
            keep = check_coverage_and_cap(env_name, control, data["leaves"], data["refs"])
            if tag != "narrow":  # the comparison itself once per control set (the other arrays differ in size and rounding only)
                continue
            env, _, _, _ = make_env(env_name, B, torch.float64, control_state=list(control), device="cpu")
            states = make_states(env, data)
            got = to_np(env.vmap_reward_vjp(states, tensor(data["g"])[..., None]), fields)
            want = oracle_grads(env_name, control, data["leaves"], data["refs"], data["g"])
            assert [g is not None for g in got] == expected_reads(env_name, control), control
            for n, g, w in zip(fields, got, want):
                if w is None:
                    continue
                assert g.shape == (B, ROWS) and np.all(g[:, 0] == 0)
                assert np.abs(w).max() > 0
                d = rel_dist(g, w, keep)
                worst = max(worst, d)
                assert d <= 1e-7, (control, n, d)
    print(f"{env_name}: worst rel dist {worst:.3e}")


def test_cpu_reward_vjp_takes_a_two_dimensional_cotangent_and_ignores_the_switch():
    control = ("theta",)
    data = reward_inputs("pendulum", control, NARROW_B, ROWS, 8)
    env, _, _, _ = make_env("pendulum", NARROW_B, torch.float64, control_state=list(control), device="cpu")
    states = make_states(env, data)
    a = env.vmap_reward_vjp(states, tensor(data["g"]))
    env.differentiable = True
    b = env.vmap_reward_vjp(states, tensor(data["g"])[..., None])
    assert torch.equal(a.theta, b.theta) and a.omega is None and b.omega is None


# ---------------------------------------------------------------------------------------------------------------- 5
def test_rew_vjp_kernels_use_no_scratch():
    res = budget("rew_vjp_kernel")[0]
    assert len(res) == 6 * 2 * 2, len(res)  # six models x two element types x two forms
    assert not any("sim_ahead_vjp_kernel" in k for k in res)
    over = {k: v for k, v in res.items() if v["scratch"] != 0}
    assert not over, over
