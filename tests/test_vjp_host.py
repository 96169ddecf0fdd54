"""Host side of the reverse mode (no GPU): the C ABI declares and exports excenv_sim_ahead_vjp, rejects what has no reverse mode
before any launch, the built sim_ahead_vjp_kernel instantiations stay within the register / scratch / loop-size budget, and the
Python switch defaults to off."""
import ctypes
import os
import re

import pytest
import torch

from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget, check_budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4


def test_header_declares_and_library_exports_the_vjp_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_sim_ahead_vjp\s*\(", hdr)
    assert re.search(r"\bint64_t\s+excenv_sim_ahead_vjp_workspace_bytes\s*\(", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # an addition: a binder probes for the symbol
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_sim_ahead_vjp") and hasattr(lib, "excenv_sim_ahead_vjp_workspace_bytes")
    assert "excenv_sim_ahead_vjp" in _native.PROTOTYPES and len(_native.PROTOTYPES["excenv_sim_ahead_vjp"][1]) == 23
    wb = _native.lib().excenv_sim_ahead_vjp_workspace_bytes
    assert wb(5, 0, 1000, 10, _native.LAYOUT_LANE_MAJOR) == 0
    assert wb(5, 0, 1000, 10, _native.LAYOUT_ENV_MAJOR) == (4 * 10 * 2 * 1000 + 255) // 256 * 256
    assert wb(17, 0, 1000, 10, 0) == -1
    # the size for a given call: the tank under "ahead" with an RK solver adds the raw levels [K * substeps + 1][B]
    assert re.search(r"\bint64_t\s+excenv_sim_ahead_vjp_workspace_bytes_for\s*\(", hdr)
    wbf = _native.lib().excenv_sim_ahead_vjp_workspace_bytes_for
    up = lambda n: (n + 255) // 256 * 256
    lm, em = _native.LAYOUT_LANE_MAJOR, _native.LAYOUT_ENV_MAJOR
    assert wbf(4, 1, _native.F64, 1000, 10, 3, _native.SEM_AHEAD, lm) == up(8 * 31 * 1000)
    assert wbf(4, 2, _native.F32, 1000, 10, 1, _native.SEM_AHEAD, em) == up(4 * 10 * 1000) + up(4 * 11 * 1000)
    assert wbf(4, 0, _native.F64, 1000, 10, 3, _native.SEM_AHEAD, lm) == 0  # Euler: the stage state is the saved row
    assert wbf(4, 1, _native.F64, 1000, 10, 3, _native.SEM_STEP, lm) == 0   # "step" carries the post-processed state
    for env in (0, 1, 2, 3, 5):
        assert wbf(env, 2, _native.F32, 1000, 10, 1, _native.SEM_AHEAD, em) == wb(env, _native.F32, 1000, 10, em)
    assert wbf(17, 0, 0, 1000, 10, 1, _native.SEM_AHEAD, lm) == -1 and wbf(4, 1, 0, 1000, 10, 0, _native.SEM_AHEAD, lm) == -1


def _call(env=0, solver=0, dtype=0, B=4, K=3, sub=1, props=None, semantics=_native.SEM_AHEAD, layout=_native.LAYOUT_LANE_MAJOR,
          opts=None, ws=None, ws_bytes=0):
    lib = _native.lib()
    p = props if props is not None else _native.Props()
    one = (ctypes.c_void_p * 8)(*([64] * 8))
    rc = lib.excenv_sim_ahead_vjp(env, solver, dtype, i64(B), i64(K), i32(sub), ctypes.byref(p), None, dbl(1e-4), dbl(1e-4), vp(64),
                                  layout, one, vp(64), one, one, vp(64), one, semantics, ws, i64(ws_bytes),
                                  None if opts is None else ctypes.byref(opts), None)
    return rc, lib.excenv_last_error()


def test_unsupported_combinations_are_rejected_before_any_launch():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    # the saturated PMSM
    p = _native.Props()
    lut = _native.PmsmLut(4, 4, 64, 64, 64)
    p.pmsm_lut = ctypes.pointer(lut)
    rc, msg = _call(env=5, props=p)
    assert rc == EUNSUPPORTED and b"saturated" in msg
    # the accumulated-time clock
    rc, msg = _call(semantics=_native.SEM_AHEAD_ACCUMULATED_T)
    assert rc == EUNSUPPORTED and b"ACCUMULATED_T" in msg
    # a [B] property leaf
    p = _native.Props()
    p.static_params[1].per_env = 64
    rc, msg = _call(props=p)
    assert rc == EUNSUPPORTED and b"per-environment" in msg
    p = _native.Props()
    p.state_max[0].per_env = 64
    rc, msg = _call(props=p)
    assert rc == EUNSUPPORTED and msg
    # the tiled layout
    rc, msg = _call(layout=_native.LAYOUT_TILED)
    assert rc == EUNSUPPORTED and b"tiled" in msg
    # bad values
    assert _call(env=9)[0] == EINVAL
    assert _call(semantics=7)[0] == EINVAL
    assert _call(K=-1)[0] == EINVAL
    assert _call(sub=0)[0] == EINVAL
    rc, msg = _call(layout=_native.LAYOUT_ENV_MAJOR)  # row-major actions without their workspace
    assert rc == EINVAL and b"workspace" in msg
    rc, msg = _call(env=4, solver=1)  # the tank, RK4, "ahead": the raw levels need their workspace
    assert rc == EINVAL and b"excenv_sim_ahead_vjp_workspace_bytes_for" in msg
    rc, msg = _call(env=4, solver=1, ws=vp(256), ws_bytes=255)
    assert rc == EINVAL and b"256 bytes" in msg  # B = 4, K = 3, fp32: 4 * 4 * 4 = 64 -> 256
    rc, msg = _call(opts=_native.LaunchOpts(2, 0, 0, 0))  # fp32: the forms are 1 and 4 environments per lane
    assert rc == EINVAL and b"envs_per_lane" in msg
    rc, msg = _call(env=3, solver=2, opts=_native.LaunchOpts(4, 0, 0, 0))  # acrobot Tsit5 has the one-environment form only
    assert rc == EINVAL and b"envs_per_lane" in msg
    lib = _native.lib()
    p = _native.Props()
    rc = lib.excenv_sim_ahead_vjp(0, 0, 0, i64(4), i64(3), i32(1), ctypes.byref(p), None, dbl(1e-4), dbl(1e-4), vp(64), 1, None,
                                  None, None, None, vp(64), None, 1, None, i64(0), None, None)
    assert rc == ENULL and lib.excenv_last_error()


def test_vjp_kernels_stay_within_the_register_scratch_and_loop_budget():
    """tools/loop_code_size.py on the built library: every sim_ahead_vjp_kernel instantiation uses no scratch memory and at most 256
    vector registers (accumulation registers included), and its largest loop is below 60 KB — the bound of the headline test."""
    res, spans = budget("sim_ahead_vjp_kernel")
    # six models x three solvers x two semantics x two dtypes, one environment per lane; the wide forms on top
    assert len(res) >= 72 + 30, len(res)
    check_budget(res, spans)


def test_differentiable_defaults_to_false():
    for reg in EnvironmentRegistry:
        env = reg.make(batch_size=4, device="cpu")
        assert env.differentiable is False
    env.differentiable = True
    assert env.differentiable is True


def test_python_rejects_what_has_no_reverse_mode_by_name():
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    _, state = env.vmap_reset()
    actions = torch.zeros(4, 3, 1)
    for attr, value, word in (("sim_ahead_semantics", "ahead_accumulated_t", "ahead_accumulated_t"), ("traj_layout", "env_major", "env_major"),
                              ("traj_layout", "tiled", "tiled")):
        env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
        setattr(env, attr, value)
        with pytest.raises(ValueError, match=word):
            env.vmap_sim_ahead_vjp(None, actions, 1e-4, 1e-4)
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", static_params={"g": torch.full((4,), 9.81), "l": 1.0, "m": 1.0})
    with pytest.raises(ValueError, match="per-environment"):
        env.vmap_sim_ahead_vjp(None, actions, 1e-4, 1e-4)
    # out= and gym outputs cannot be combined with a differentiable call
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    env.differentiable = True
    _, state = env.vmap_reset()
    a = torch.zeros(4, 3, 1, requires_grad=True)
    with pytest.raises(ValueError, match="out="):
        env.vmap_sim_ahead(state, a, 1e-4, 1e-4, out=(None, None, None))
    with pytest.raises(ValueError, match="return_rew_trunc_term"):
        env.vmap_sim_ahead(state, a, 1e-4, 1e-4, return_rew_trunc_term=True)


def test_vjp_form_rule_is_the_forwards_batch_rule(tmp_path):
    """vjp.hpp is host-only: the host compiler builds its constexpr functions alone (static_asserts are the test)"""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('''#include "vjp.hpp"
using namespace excenv;
static_assert(vjp_envs_per_lane(EXCENV_PMSM, EXCENV_EULER, 1 << 19, 4, 0, true) == 4, "the forward's rule: four per lane from 2^19");
static_assert(vjp_envs_per_lane(EXCENV_PMSM, EXCENV_EULER, 1 << 18, 4, 0, true) == 1, "");
static_assert(vjp_envs_per_lane(EXCENV_PMSM, EXCENV_EULER, 1 << 19, 4, 0, false) == 1, "unaligned: one per lane");
static_assert(vjp_envs_per_lane(EXCENV_PMSM, EXCENV_EULER, 256, 4, 4, true) == 4, "forced");
static_assert(vjp_envs_per_lane(EXCENV_PMSM, EXCENV_EULER, 256, 4, 2, true) == 0, "no two-per-lane form in fp32");
static_assert(vjp_envs_per_lane(EXCENV_ACROBOT, EXCENV_TSIT5, 1 << 20, 4, 0, true) == 1, "");
static_assert(vjp_envs_per_lane(EXCENV_PENDULUM, EXCENV_TSIT5, 1 << 20, 8, 0, true) == 2, "");
static_assert(vjp_instantiated(EXCENV_SEM_AHEAD, EXCENV_PMSM, 4, EXCENV_EULER, false, 4), "");
static_assert(!vjp_instantiated(EXCENV_SEM_AHEAD, EXCENV_PMSM, 4, EXCENV_EULER, true, 1), "saturated PMSM");
static_assert(!vjp_instantiated(EXCENV_SEM_AHEAD_ACCUMULATED_T, EXCENV_PENDULUM, 4, EXCENV_EULER, false, 1), "");
static_assert(vjp_workspace_bytes(2, 4, 1000, 10, EXCENV_LAYOUT_LANE_MAJOR) == 0, "");
static_assert(vjp_needs_raw_rows(EXCENV_FLUID_TANK, EXCENV_TSIT5, EXCENV_SEM_AHEAD), "");
static_assert(!vjp_needs_raw_rows(EXCENV_FLUID_TANK, EXCENV_EULER, EXCENV_SEM_AHEAD), "");
static_assert(!vjp_needs_raw_rows(EXCENV_FLUID_TANK, EXCENV_RK4, EXCENV_SEM_STEP), "");
static_assert(!vjp_needs_raw_rows(EXCENV_PENDULUM, EXCENV_RK4, EXCENV_SEM_AHEAD), "");
static_assert(vjp_raw_rows_bytes(EXCENV_FLUID_TANK, EXCENV_RK4, EXCENV_SEM_AHEAD, 8, 1000, 10, 3) == 248064, "31 rows, 256-byte units");
int main() { return 0; }
''')
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "exciting-environments_amd", "csrc"), "-fsyntax-only", str(src)], check=True)
