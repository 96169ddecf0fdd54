"""What the reverse-mode entry points refuse before any launch (no GPU, fake pointers): one table of faults over
excenv_sim_ahead_vjp, excenv_sim_ahead_vjp_params, excenv_step_vjp and excenv_step_jacobian, and excenv_rew_vjp where it makes the
same check. Each row pins the return code and the whole message; the double faults pin which check comes first."""
import ctypes

import pytest

from exciting_environments_amd import _native

i64, vp, dbl = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL, EUNSUPPORTED = -1, -2, -4
GROUPS = ("static_params", "state_min", "state_max", "action_min", "action_max")

# fault -> what the call is made with: props (None = NULL), lut, per_env (a property group), nc (n_control), epl (envs_per_lane), B
FAULTS = {
    "null_props": dict(props=None),
    "lut": dict(lut=True),
    **{f"per_env_{g}": dict(per_env=g) for g in GROUPS},
    "n_control_-1": dict(nc=-1),
    "n_control_9": dict(nc=_native.MAX_CONTROL + 1),
    "epl_3": dict(epl=3),
    "B_-1": dict(B=-1),
    "lut+per_env": dict(lut=True, per_env="static_params"),
    "null_props+epl_3": dict(props=None, epl=3),
    "n_control_9+lut": dict(nc=_native.MAX_CONTROL + 1, lut=True),
}


def _ptrs():
    return (ctypes.c_void_p * 9)(*([64] * 9))


def _call(fn, props="default", lut=False, per_env=None, nc=0, epl=0, B=4):
    """One call of `fn` with fake 16-byte aligned addresses everywhere; PMSM where the tables are attached, else the pendulum."""
    lib = _native.lib()
    env = 5 if lut else 0
    keep = []
    if props == "default":
        props = _native.Props()
        if lut:
            keep.append(_native.PmsmLut(4, 4, 64, 64, 64))
            props.pmsm_lut = ctypes.pointer(keep[0])
        if per_env:
            getattr(props, per_env)[0].per_env = 64
    p = None if props is None else ctypes.byref(props)
    control = None
    if nc:
        control = _native.Control()
        control.n_control = nc
        for j in range(_native.MAX_CONTROL):
            control.reference[j] = 64
    c = None if control is None else ctypes.byref(control)
    opts = _native.LaunchOpts(epl, 0, 0, 0)
    o = ctypes.byref(opts)
    if fn in ("excenv_sim_ahead_vjp", "excenv_sim_ahead_vjp_params"):
        args = [env, 0, 0, i64(B), i64(2), 1, p, c, dbl(1e-2), dbl(1e-2), vp(64), _native.LAYOUT_LANE_MAJOR, _ptrs(), vp(64), None, None,
                vp(64), _ptrs(), _native.SEM_STEP, None, i64(0), o, None]
        if fn.endswith("_params"):
            args.append((ctypes.c_void_p * 9)(64))  # the gradient of the first static parameter
        rc = getattr(lib, fn)(*args)
    elif fn == "excenv_step_vjp":
        rc = lib.excenv_step_vjp(env, 0, 0, i64(B), p, c, dbl(1e-2), _ptrs(), vp(64), _ptrs(), vp(64), None, None, _ptrs(), vp(64), o, None)
    elif fn == "excenv_step_jacobian":
        rc = lib.excenv_step_jacobian(env, 0, 0, i64(B), i64(2), 1, p, nc, dbl(1e-2), dbl(1e-2), _ptrs(), _ptrs(), i64(B), vp(64), i64(B),
                                      i64(2 * B), i64(1), _native.JAC_STATE, vp(64), o, None)
    else:  # excenv_rew_vjp: two lane-major rows, so that only the fault keeps the call from its 16-byte form
        rc = lib.excenv_rew_vjp(env, 0, i64(B), i64(2), p, c, None, _ptrs(), i64(1), i64(B), vp(64), i64(1), i64(B), _ptrs(), o, None)
    return rc, lib.excenv_last_error().decode()


# entry point, fault, further arguments of the call, return code, message
TABLE = [
    ("excenv_sim_ahead_vjp", "null_props", {}, ENULL, 'excenv_sim_ahead_vjp: NULL argument'),
    ("excenv_sim_ahead_vjp", "lut", {}, EUNSUPPORTED, 'excenv_sim_ahead_vjp: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_sim_ahead_vjp", "per_env_static_params", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp", "per_env_state_min", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp", "per_env_state_max", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp", "per_env_action_min", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp", "per_env_action_max", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp", "n_control_-1", {}, EINVAL, 'excenv_sim_ahead_vjp: bad n_control -1'),
    ("excenv_sim_ahead_vjp", "n_control_9", {}, EINVAL, 'excenv_sim_ahead_vjp: bad n_control 9'),
    ("excenv_sim_ahead_vjp", "epl_3", {}, EINVAL, 'excenv_sim_ahead_vjp: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)'),
    ("excenv_sim_ahead_vjp", "B_-1", {}, EINVAL, 'excenv_sim_ahead_vjp: bad batch size -1'),
    ("excenv_sim_ahead_vjp", "lut+per_env", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_sim_ahead_vjp", "null_props+epl_3", {}, ENULL, 'excenv_sim_ahead_vjp: NULL argument'),
    ("excenv_sim_ahead_vjp", "n_control_9+lut", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_sim_ahead_vjp_params", "null_props", {}, ENULL, 'excenv_sim_ahead_vjp_params: NULL argument'),
    ("excenv_sim_ahead_vjp_params", "lut", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_sim_ahead_vjp_params", "per_env_static_params", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp_params", "per_env_state_min", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp_params", "per_env_state_max", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp_params", "per_env_action_min", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp_params", "per_env_action_max", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_sim_ahead_vjp_params", "n_control_-1", {}, EINVAL, 'excenv_sim_ahead_vjp_params: bad n_control -1'),
    ("excenv_sim_ahead_vjp_params", "n_control_9", {}, EINVAL, 'excenv_sim_ahead_vjp_params: bad n_control 9'),
    ("excenv_sim_ahead_vjp_params", "epl_3", {}, EINVAL,
     'excenv_sim_ahead_vjp_params: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)'),
    ("excenv_sim_ahead_vjp_params", "B_-1", {}, EINVAL, 'excenv_sim_ahead_vjp_params: bad batch size -1'),
    ("excenv_sim_ahead_vjp_params", "lut+per_env", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_sim_ahead_vjp_params", "null_props+epl_3", {}, ENULL, 'excenv_sim_ahead_vjp_params: NULL argument'),
    ("excenv_sim_ahead_vjp_params", "n_control_9+lut", {}, EUNSUPPORTED,
     'excenv_sim_ahead_vjp_params: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_step_vjp", "null_props", {}, ENULL, 'excenv_step_vjp: props is NULL'),
    ("excenv_step_vjp", "lut", {}, EUNSUPPORTED, 'excenv_step_vjp: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_step_vjp", "per_env_static_params", {}, EUNSUPPORTED,
     'excenv_step_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_vjp", "per_env_state_min", {}, EUNSUPPORTED,
     'excenv_step_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_vjp", "per_env_state_max", {}, EUNSUPPORTED,
     'excenv_step_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_vjp", "per_env_action_min", {}, EUNSUPPORTED,
     'excenv_step_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_vjp", "per_env_action_max", {}, EUNSUPPORTED,
     'excenv_step_vjp: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_vjp", "n_control_-1", {}, EINVAL, 'excenv_step_vjp: bad n_control -1'),
    ("excenv_step_vjp", "n_control_9", {}, EINVAL, 'excenv_step_vjp: bad n_control 9'),
    ("excenv_step_vjp", "epl_3", {}, EINVAL, 'excenv_step_vjp: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)'),
    ("excenv_step_vjp", "B_-1", {}, EINVAL, 'excenv_step_vjp: bad batch size -1'),
    ("excenv_step_vjp", "lut+per_env", {}, EUNSUPPORTED, 'excenv_step_vjp: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_step_vjp", "null_props+epl_3", {}, ENULL, 'excenv_step_vjp: props is NULL'),
    ("excenv_step_vjp", "n_control_9+lut", {}, EUNSUPPORTED, 'excenv_step_vjp: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_step_jacobian", "null_props", {}, ENULL, 'excenv_step_jacobian: props is NULL'),
    ("excenv_step_jacobian", "lut", {}, EUNSUPPORTED, 'excenv_step_jacobian: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_step_jacobian", "per_env_static_params", {}, EUNSUPPORTED,
     'excenv_step_jacobian: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_jacobian", "per_env_state_min", {}, EUNSUPPORTED,
     'excenv_step_jacobian: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_jacobian", "per_env_state_max", {}, EUNSUPPORTED,
     'excenv_step_jacobian: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_jacobian", "per_env_action_min", {}, EUNSUPPORTED,
     'excenv_step_jacobian: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_jacobian", "per_env_action_max", {}, EUNSUPPORTED,
     'excenv_step_jacobian: per-environment property arrays are not supported (broadcast properties only)'),
    ("excenv_step_jacobian", "n_control_-1", {}, EINVAL, 'excenv_step_jacobian: bad n_control -1'),
    ("excenv_step_jacobian", "n_control_9", {}, EINVAL, 'excenv_step_jacobian: bad n_control 9'),
    ("excenv_step_jacobian", "epl_3", {}, EINVAL, 'excenv_step_jacobian: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)'),
    ("excenv_step_jacobian", "B_-1", {}, EINVAL, 'excenv_step_jacobian: bad batch size -1'),
    ("excenv_step_jacobian", "lut+per_env", {}, EUNSUPPORTED,
     'excenv_step_jacobian: the saturated PMSM (pmsm_lut) has no reverse mode'),
    ("excenv_step_jacobian", "null_props+epl_3", {}, ENULL, 'excenv_step_jacobian: props is NULL'),
    ("excenv_step_jacobian", "n_control_9+lut", {}, EINVAL, 'excenv_step_jacobian: bad n_control 9'),
    ("excenv_rew_vjp", "null_props", {}, ENULL, 'excenv_rew_vjp: NULL argument'),
    ("excenv_rew_vjp", "per_env_static_params", {'epl': 4}, EINVAL,
     'excenv_rew_vjp: opts.envs_per_lane = 4 is not available (1, or 4 with lane-major 16-byte aligned arrays, batch_size % 4 == 0 and broadcast properties)'),
    ("excenv_rew_vjp", "per_env_state_min", {'epl': 4}, EINVAL,
     'excenv_rew_vjp: opts.envs_per_lane = 4 is not available (1, or 4 with lane-major 16-byte aligned arrays, batch_size % 4 == 0 and broadcast properties)'),
    ("excenv_rew_vjp", "per_env_state_max", {'epl': 4}, EINVAL,
     'excenv_rew_vjp: opts.envs_per_lane = 4 is not available (1, or 4 with lane-major 16-byte aligned arrays, batch_size % 4 == 0 and broadcast properties)'),
    ("excenv_rew_vjp", "per_env_action_min", {'epl': 4}, EINVAL,
     'excenv_rew_vjp: opts.envs_per_lane = 4 is not available (1, or 4 with lane-major 16-byte aligned arrays, batch_size % 4 == 0 and broadcast properties)'),
    ("excenv_rew_vjp", "per_env_action_max", {'epl': 4}, EINVAL,
     'excenv_rew_vjp: opts.envs_per_lane = 4 is not available (1, or 4 with lane-major 16-byte aligned arrays, batch_size % 4 == 0 and broadcast properties)'),
    ("excenv_rew_vjp", "n_control_-1", {}, EINVAL, 'excenv_rew_vjp: bad n_control -1'),
    ("excenv_rew_vjp", "n_control_9", {}, EINVAL, 'excenv_rew_vjp: bad n_control 9'),
    ("excenv_rew_vjp", "epl_3", {}, EINVAL, 'excenv_rew_vjp: opts.envs_per_lane must be 0, 1, 2 or 4 (got 3)'),
    ("excenv_rew_vjp", "B_-1", {}, EINVAL, 'excenv_rew_vjp: bad batch size -1'),
    ("excenv_rew_vjp", "null_props+epl_3", {}, ENULL, 'excenv_rew_vjp: NULL argument'),
]


@pytest.mark.parametrize("fn,fault,extra,rc,message", TABLE, ids=[f"{r[0]}-{r[1]}" for r in TABLE])
def test_the_refusal_comes_back_by_code_and_whole_message(fn, fault, extra, rc, message):
    assert _call(fn, **FAULTS[fault], **extra) == (rc, message)


def test_the_table_covers_every_fault_of_every_reverse_entry_point():
    """The four reverse entry points meet every fault; excenv_rew_vjp the ones whose check it shares (a valid pmsm_lut is not read
    there, and per-environment arrays only rule out its 16-byte form: asked for by envs_per_lane = 4)."""
    seen = {(r[0], r[1]) for r in TABLE}
    for fn in ("excenv_sim_ahead_vjp", "excenv_sim_ahead_vjp_params", "excenv_step_vjp", "excenv_step_jacobian"):
        assert {f for f in FAULTS if (fn, f) not in seen} == set(), fn
    shared = {f for f in FAULTS if "lut" not in f}
    assert {f for f in shared if ("excenv_rew_vjp", f) not in seen} == set()
