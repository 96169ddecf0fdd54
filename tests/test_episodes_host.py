"""Host side of the episode rollouts (no GPU): the header declares excenv_sim_policy_episodes and _native mirrors it, the entry point
refuses by code and whole message what it does not do before any launch (in excenv_sim_policy's order, then the episode record), an
empty batch makes no launch, `vmap_rollout_episodes` raises the named exceptions on CPU environments, every built sim_episodes_kernel
instantiation is free of scratch memory and static LDS (or is listed by name), the numpy restatement of the reset rule is the
written contract on a hand-computed example, and the inputs E1 / E2 of the GPU suite end episodes for every reason, neither never nor
always, on the float64 oracle loop alone."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget
import helpers_episodes as he

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, i32, vp, dbl = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_double
EINVAL, ENULL = -1, -2
MODELS = ["Pendulum", "MassSpringDamper", "CartPole", "Acrobot", "FluidTank", "Pmsm", "PmsmSat"]
FN = "excenv_sim_policy_episodes"


def test_header_declares_native_mirrors_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"\bint\s+excenv_sim_policy_episodes\s*\(", hdr)
    assert re.search(r"\}\s*excenv_episode_t\s*;", hdr)
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)  # an addition: a binder probes for the symbol
    assert re.search(r"#define\s+EXCENV_END_TERMINATED\s+1\b", hdr) and re.search(r"#define\s+EXCENV_END_TRUNCATED\s+2\b", hdr)
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "excenv_sim_policy_episodes")
    assert lib.excenv_abi_version() == 7 and _native.ABI_VERSION == 7
    # excenv_sim_policy's arguments and the record, behind actions_out
    assert len(_native.PROTOTYPES["excenv_sim_policy_episodes"][1]) == len(_native.PROTOTYPES["excenv_sim_policy"][1]) + 1 == 19
    assert _native.STRUCTS[_native.Episode] == "excenv_episode_t"
    assert [f[0] for f in _native.Episode._fields_] == ["reset_states", "n_reset_rows", "end_mask", "max_episode_steps", "episode_steps_in",
                                                        "reward", "terminated", "truncated", "reset", "n_resets", "episode_steps_out"]
    assert (_native.END_TERMINATED, _native.END_TRUNCATED) == (1, 2)
    assert _native.END_ON == {"terminated": 1, "truncated": 2}


# ---- refusals: fake 16-byte aligned addresses everywhere, nothing may reach a launch ----------------------------------------------
def _call(env=0, B=4, K=2, substeps=1, policy="default", episode="default", null=None, epl=0, widths=(2, 8, 1), n_layers=None,
          activation=1, n_control=0, lut=False, **fields):
    """One excenv_sim_policy_episodes call (pendulum: S = 2, O = 2, A = 1). null: the argument (or record field) passed as NULL;
    fields: policy / episode fields"""
    lib = _native.lib()
    props = _native.Props()
    keep = []
    if lut:
        keep.append(_native.PmsmLut(4, 4, 64, 64, 64))
        props.pmsm_lut = ctypes.pointer(keep[0])
    ptrs = lambda: (ctypes.c_void_p * 8)(*([64] * 8))
    a = dict(state_in=ptrs(), obs_traj=vp(64), state_traj=ptrs(), last_state=ptrs(), actions_out=vp(64), reset_states=ptrs())
    f = dict(params=64, noise=None, clip_lo=-1.0, clip_hi=1.0, n_reset_rows=2, end_mask=3, max_episode_steps=5, episode_steps_in=64,
             reward=64, terminated=64, truncated=64, reset=64, n_resets=64, episode_steps_out=64)
    f.update(fields)
    if null in a:
        a[null] = None
    elif null in f:
        f[null] = None
    elif null is not None:  # "reset_states[1]": one entry of a pointer array
        name, j = null[:-3], int(null[-2])
        a[name][j] = None
    w = (ctypes.c_int32 * 5)(*(tuple(widths) + (0,) * (5 - len(widths))))
    p = _native.Policy(f["params"], len(widths) - 1 if n_layers is None else n_layers, activation, w, f["noise"], f["clip_lo"], f["clip_hi"])
    rs = None if a["reset_states"] is None else ctypes.addressof(a["reset_states"])
    e = _native.Episode(rs, f["n_reset_rows"], f["end_mask"], f["max_episode_steps"], f["episode_steps_in"], f["reward"], f["terminated"],
                        f["truncated"], f["reset"], f["n_resets"], f["episode_steps_out"])
    control = None
    if n_control:
        control = _native.Control(n_control, (ctypes.c_int32 * 8)(*([0] * 8)), (ctypes.c_void_p * 8)(*([64] * 8)), (ctypes.c_void_p * 8)())
    opts = _native.LaunchOpts(epl, 0, 0, 0)
    rc = lib.excenv_sim_policy_episodes(env, 0, 0, i64(B), i64(K), i32(substeps), ctypes.byref(props),
                                        None if control is None else ctypes.byref(control), dbl(1e-4), dbl(1e-4), a["state_in"],
                                        None if policy is None else ctypes.byref(p), a["obs_traj"], a["state_traj"], a["last_state"],
                                        a["actions_out"], None if episode is None else ctypes.byref(e), ctypes.byref(opts), None)
    return rc, lib.excenv_last_error().decode()


# what the call is made with, return code, the whole message: excenv_sim_policy's refusals under this entry's name, in its order ...
REFUSALS = [
    (dict(K=-1), EINVAL, f"{FN}: bad K=-1 or substeps=1"),
    (dict(substeps=0), EINVAL, f"{FN}: bad K=2 or substeps=0"),
    (dict(B=-1), EINVAL, f"{FN}: bad batch size -1"),
    (dict(env=7), EINVAL, f"{FN}: bad env id 7"),
    (dict(null="obs_traj"), ENULL, f"{FN}: obs_traj is NULL"),
    (dict(null="last_state"), ENULL, f"{FN}: last_state is NULL"),
    (dict(null="state_in"), ENULL, f"{FN}: state_in is NULL"),
    (dict(policy=None), ENULL, f"{FN}: policy is NULL"),
    (dict(null="params"), ENULL, f"{FN}: policy->params is NULL"),
    (dict(n_layers=5), EINVAL, f"{FN}: policy->n_layers must be 1 .. 4 (got 5)"),
    (dict(widths=(2, 65, 1)), EINVAL, f"{FN}: policy->widths[1] must be 1 .. 64 (got 65)"),
    (dict(widths=(2, 1), n_control=2), EINVAL,
     f"{FN}: policy->widths must run from the observation width 4 to the action width 1 (got 2 .. 1)"),
    (dict(activation=2), EINVAL, f"{FN}: policy->activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got 2)"),
    (dict(clip_lo=0.5, clip_hi=0.25), EINVAL,
     f"{FN}: policy->clip_lo = 0.5 and policy->clip_hi = 0.25 are not an interval (-inf / +inf: no clamp)"),
    (dict(epl=2), EINVAL, f"{FN}: opts.envs_per_lane = 2 is not available (this kernel has the one-environment-per-lane form only)"),
    (dict(env=5, substeps=2, widths=(8, 2)), EINVAL,
     f"{FN}: PMSM: obs_stepsize must equal action_stepsize (substeps = 2; reference pmsm_env.py:787)"),
    # ... then the episode record: NULL pointers first, then values
    (dict(episode=None), ENULL, f"{FN}: episode is NULL"),
    (dict(null="reset_states"), ENULL, f"{FN}: episode->reset_states is NULL"),
    (dict(null="reset_states[0]"), ENULL, f"{FN}: episode->reset_states pointer 0 is NULL"),
    (dict(null="reset_states[1]"), ENULL, f"{FN}: episode->reset_states pointer 1 is NULL"),
    (dict(substeps=2), EINVAL, f"{FN}: substeps must be 1 (one solver step per action, as GymWrapper.step does; got 2)"),
    (dict(substeps=3, n_reset_rows=0), EINVAL, f"{FN}: substeps must be 1 (one solver step per action, as GymWrapper.step does; got 3)"),
    (dict(n_reset_rows=0), EINVAL, f"{FN}: episode->n_reset_rows must be at least 1 (got 0)"),
    (dict(n_reset_rows=-2), EINVAL, f"{FN}: episode->n_reset_rows must be at least 1 (got -2)"),
    (dict(end_mask=4), EINVAL, f"{FN}: episode->end_mask has unknown bits (got 4; EXCENV_END_TERMINATED = 1, EXCENV_END_TRUNCATED = 2)"),
    (dict(end_mask=-1), EINVAL, f"{FN}: episode->end_mask has unknown bits (got -1; EXCENV_END_TERMINATED = 1, EXCENV_END_TRUNCATED = 2)"),
    (dict(max_episode_steps=-1), EINVAL, f"{FN}: episode->max_episode_steps must not be negative (got -1; 0: no time limit)"),
    (dict(end_mask=0, max_episode_steps=0), EINVAL,
     f"{FN}: episode->end_mask = 0 and episode->max_episode_steps = 0: nothing can end an episode (use excenv_sim_policy)"),
    # the record is judged before the model is chosen, and the leaves behind it at the launch
    (dict(env=0, lut=True), EINVAL, "pmsm_lut is only valid for EXCENV_PMSM"),
    (dict(null="last_state[1]"), ENULL, f"{FN}: state pointer 1 is NULL"),
    (dict(null="state_traj[0]"), ENULL, f"{FN}: state_traj pointer 0 is NULL"),
    # an earlier refusal wins over a later one
    (dict(policy=None, episode=None), ENULL, f"{FN}: policy is NULL"),
    (dict(epl=4, episode=None), EINVAL, f"{FN}: opts.envs_per_lane = 4 is not available (this kernel has the one-environment-per-lane form only)"),
]


@pytest.mark.parametrize("how,rc,message", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in REFUSALS])
def test_the_refusal_comes_back_by_code_and_whole_message(how, rc, message):
    assert _call(**how) == (rc, message)


def test_an_empty_batch_is_ok_without_a_launch():
    """B == 0: nothing to do — and no GPU here, so a launch would have come back as EXCENV_EHIP. Every optional output may be NULL."""
    assert _call(B=0)[0] == 0
    assert _call(B=0, K=0, widths=(2, 1))[0] == 0
    assert _call(B=0, end_mask=0, reward=None, terminated=None, truncated=None, reset=None, n_resets=None, episode_steps_out=None,
                 episode_steps_in=None)[0] == 0
    assert _call(B=0, max_episode_steps=0, end_mask=2)[0] == 0


def test_sim_episodes_kernels_exist_and_use_no_scratch():
    """tools/loop_code_size.py kernel_resources on the built library: the 42 instantiations (seven models, the saturated PMSM
    included, x three solvers x two element types) are all there; any with a private segment or static LDS is listed by name with
    its bytes, and there is none. The 42 sim_policy_kernel instantiations next to them are still 42."""
    res, spans = budget("sim_episodes_kernel")
    for model, t, solver in itertools.product(MODELS, "fd", (0, 1, 2)):
        key = f"sim_episodes_kernelINS_{len(model)}{model}I{t}EE{t}Li{solver}EE"
        hit = [k for k in res if key in k]
        assert len(hit) == 1, (key, hit)
        print(f"{model} {'fp32' if t == 'f' else 'fp64'} solver {solver}: {res[hit[0]]} loop {spans[hit[0]][0]} B of {spans[hit[0]][1]} B")
    assert len(res) == 42, len(res)
    spilled = {k: (v["scratch"], v["lds"]) for k, v in res.items() if v["scratch"] or v["lds"]}
    for k, (scratch, lds) in sorted(spilled.items()):
        print(f"{k}: {scratch} B of scratch per lane, {lds} B of static LDS")
    assert not spilled, spilled
    assert max(v[0] for v in spans.values()) < 60 * 1024  # the trajectory loop stays inside the instruction cache
    assert len(budget("sim_policy_kernel")[0]) == 42


# ---- the reset rule, restated ---------------------------------------------------------------------------------------------------------
def test_reset_rule_restatement_is_the_written_contract():
    """helpers_episodes.reset_rule_np on three rows of four environments, every entry worked out by hand from the contract:
    end_n = (terminated and bit 1) or (truncated and bit 2) or (max > 0 and t_n >= max); t_{n+1} = end_n ? 0 : t_n + 1"""
    term = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 0, 0]], bool)
    trunc = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]], bool)
    t_in = [0, 5, 1, 2]
    # max = 2, both bits. env 0: t = 0, 1, 2 -> the limit ends row 2; t_out = 0. env 1: row 0 terminated (and over the limit: not
    # time-ONLY), t = 0, 1 -> rows 1, 2: row 2 has t = 1: no; t_out = 2. env 2: t = 1 row 0; t = 2 and truncated row 1; row 2 t = 0,
    # terminated; t_out = 0. env 3: t = 2 ends row 0, t = 0, 1 -> t_out = 2.
    reset, n, t_out, time_only = he.reset_rule_np(term, trunc, t_in, 2, ("terminated", "truncated"))
    assert reset.tolist() == [[False, False, True], [True, False, False], [False, True, True], [True, False, False]]
    assert n.tolist() == [1, 1, 2, 1] and t_out.tolist() == [0, 2, 0, 2]
    assert time_only.tolist() == [[False, False, True], [False, False, False], [False, False, False], [True, False, False]]
    # only "truncated", no limit: the one truncated row
    reset, n, t_out, time_only = he.reset_rule_np(term, trunc, t_in, 0, ("truncated",))
    assert reset.tolist() == [[False] * 3, [False] * 3, [False, True, False], [False] * 3]
    assert n.tolist() == [0, 0, 1, 0] and t_out.tolist() == [3, 8, 1, 5] and not time_only.any()
    # the limit alone, end_on = (): flags are ignored
    reset, n, t_out, time_only = he.reset_rule_np(term, trunc, t_in, 3, ())
    assert reset.tolist() == [[False] * 3, [True, False, False], [False, False, True], [False, True, False]]
    assert t_out.tolist() == [3, 2, 0, 1] and (time_only == reset).all()
    # no row at all
    reset, n, t_out, _ = he.reset_rule_np(np.zeros((4, 0), bool), np.zeros((4, 0), bool), t_in, 2, ("terminated",))
    assert reset.shape == (4, 0) and n.tolist() == [0] * 4 and t_out.tolist() == t_in


# ---- the input condition, on the oracle alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ("tanh", "relu"))
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_case_e1_ends_episodes_for_every_reason_on_the_oracle(env_name, deadtime, solver, activation):
    r = he.oracle_case(env_name, deadtime, solver, "E1", activation)
    flag = float(r["flag_reset"].mean())
    timed = float(r["time_only"].mean())
    total = float(r["reset"].mean())
    never = float((r["n_resets"] == 0).mean())
    wrap = float((r["n_resets"] >= 3).mean())
    print(f"E1 {env_name} deadtime {deadtime} {solver} {activation}: flag resets {flag:.3f}, time-only {timed:.3f}, all {total:.3f}, "
          f"never reset {never:.3f}, three or more resets {wrap:.3f}")
    assert np.all(np.isfinite(r["obs"])) and np.all(np.isfinite(r["actions"]))
    assert r["obs"].shape == (he.B, he.K + 1, he.hp.obs_width(env_name, he.CONTROL[env_name]))
    # the loop is the rule: the resets recomputed from its own flag rows
    term_rows = np.concatenate([r["term0"][:, None], r["terminated"][:, :-1]], axis=1)
    _, inp = he.main_case(env_name, deadtime, "E1")
    reset, n, t_out, _ = he.reset_rule_np(term_rows, r["truncated"][:, :-1].any(axis=2), inp["steps_in"], inp["max_episode_steps"], he.END_BOTH)
    assert (reset == r["reset"]).all() and (n == r["n_resets"]).all() and (t_out == r["steps_out"]).all()
    if env_name != "fluid_tank":
        assert flag >= 0.03
        assert wrap >= 0.01
    assert timed >= 0.02
    assert total <= 0.35
    assert never >= 0.10


@pytest.mark.parametrize("activation", ("tanh", "relu"))
@pytest.mark.parametrize("solver", he.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", he.CASES)
def test_case_e2_resets_every_environment_three_times_on_the_oracle(env_name, deadtime, solver, activation):
    """With the step counters of running episodes (0 or 1 under a budget of 2) every environment resets on rows 2, 5, 8 or 1, 4, 7.
    A flag-caused end in between (PMSM: 2.4 - 3.9 % of the resets with one step of dead time, 8.2 - 10.3 % without) moves the
    schedule but not the count."""
    r = he.oracle_case(env_name, deadtime, solver, "E2", activation)
    print(f"E2 {env_name} deadtime {deadtime} {solver} {activation}: flag-caused share of the resets "
          f"{float((r['flag_reset'] & r['reset']).sum() / max(1, r['reset'].sum())):.3f}")
    assert (r["n_resets"] == 3).all(), np.bincount(r["n_resets"])


# ---- Python argument faults (CPU environments: raised before anything touches a device) ---------------------------------------------
def _cpu_env(**kw):
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu", **kw)
    _, state = env.vmap_reset()
    return env, state


def _policy(widths=(2, 3, 1), **kw):
    return excenvs.MLPPolicy([torch.zeros(d, n) for n, d in zip(widths[:-1], widths[1:])], [torch.zeros(d) for d in widths[1:]], **kw)


def test_python_refuses_by_name_what_an_episode_rollout_does_not_do():
    env, state = _cpu_env()
    pol = _policy()
    for layout in ("env_major", "tiled"):
        env.traj_layout = layout
        with pytest.raises(ValueError, match=f"vmap_rollout_episodes: traj_layout='{layout}'"):
            env.vmap_rollout_episodes(state, pol, 3, env.tau, state)
    env.traj_layout = "lane_major"
    env.sim_ahead_semantics = "ahead_accumulated_t"
    with pytest.raises(ValueError, match="vmap_rollout_episodes: sim_ahead_semantics='ahead_accumulated_t'"):
        env.vmap_rollout_episodes(state, pol, 3, env.tau, state)
    env.sim_ahead_semantics = "ahead"
    with pytest.raises(ValueError, match="vmap_rollout_episodes: end_on entry 'done': 'terminated' or 'truncated'"):
        env.vmap_rollout_episodes(state, pol, 3, env.tau, state, end_on=("truncated", "done"))
    with pytest.raises(ValueError, match=r"vmap_rollout_episodes: end_on=\(\) and max_episode_steps=0: nothing can end an episode"):
        env.vmap_rollout_episodes(state, pol, 3, env.tau, state, end_on=())
    env.differentiable = True
    with pytest.raises(ValueError, match="vmap_rollout_episodes: env.differentiable with an input that requires grad"):
        env.vmap_rollout_episodes(state, pol, 3, env.tau, state, noise=torch.zeros(4, 3, 1, requires_grad=True))
    live = _policy()
    live.params.requires_grad_()
    with pytest.raises(ValueError, match="env.differentiable with an input that requires grad"):
        env.vmap_rollout_episodes(state, live, 3, env.tau, state)
    assert env.last_policy_launch == ""


def test_python_shape_faults_are_assertion_errors_with_a_message():
    env, state = _cpu_env()
    ok = _policy()
    with pytest.raises(AssertionError, match="policy needs to be an MLPPolicy, but Tensor is given"):
        env.vmap_rollout_episodes(state, torch.zeros(1, 2), 3, env.tau, state)
    with pytest.raises(AssertionError, match=r"observation width 2 to the action width 1, but its widths are \(3, 3, 1\)"):
        env.vmap_rollout_episodes(state, _policy((3, 3, 1)), 3, env.tau, state)
    with pytest.raises(AssertionError, match="n_actions is 5, but the noise has 3 action rows"):
        env.vmap_rollout_episodes(state, ok, 5, env.tau, state, noise=torch.zeros(4, 3, 1))
    with pytest.raises(AssertionError, match="clip needs to be"):
        env.vmap_rollout_episodes(state, ok, 3, env.tau, state, clip=(1.0, -1.0))
    with pytest.raises(AssertionError, match="max_episode_steps needs to be a non-negative int32, but -1 is given"):
        env.vmap_rollout_episodes(state, ok, 3, env.tau, state, max_episode_steps=-1)
    with pytest.raises(AssertionError, match=r"episode_steps needs to be of shape \(batch_size,\) which is \(4,\), but \(3,\) is given"):
        env.vmap_rollout_episodes(state, ok, 3, env.tau, state, episode_steps=torch.zeros(3, dtype=torch.int32))
    tree = env.PhysicalState(theta=torch.zeros(4, 2), omega=torch.zeros(4, 3))
    with pytest.raises(AssertionError, match="reset_states needs to be a State, a list of States or a physical state with leaves"):
        env.vmap_rollout_episodes(state, ok, 3, env.tau, tree)
    with pytest.raises(AssertionError, match="reset_states needs at least one State"):
        env.vmap_rollout_episodes(state, ok, 3, env.tau, [])
    # everything in order, in each form of reset_states: what is left is the device, by name (there is no CPU fallback)
    for rs in (state, [state, state, state], env.PhysicalState(theta=torch.zeros(4, 2), omega=torch.zeros(4, 2))):
        with pytest.raises(RuntimeError, match="vmap_rollout_episodes: tensors must live on a HIP device"):
            env.vmap_rollout_episodes(state, ok, 3, env.tau, rs, max_episode_steps=2, episode_steps=[0, 1, 2, 3])
