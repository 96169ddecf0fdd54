"""The reverse-mode kernels off the fast paths (``-m gpu``): unwrapped and huge angles in the initial state, in mixed and uniform waves.

Inputs and references are tests/helpers_cold.py's (tests/test_cold_paths_host.py runs the twin on them without a GPU, asserts the
kink cap and prints the twin's own spread). Pendulum, cart-pole, acrobot and PMSM with dead time 0 and 1; three solvers; both number
formats; B = V * 326, K = 3, substeps 1 and 2 (PMSM: 1). The special environments (helpers_cold.special_envs) hold `turns`,
`trig32`, `mod`, `quad64` (fp64) on the angle leaves and `zero` on the last leaf. Kernels: sim_ahead_vjp_kernel under both semantics
at V = 1 and every wide form of helpers_vjp.WIDE_CASES for these models, its PGRAD form (param_grads="per_env"), step_vjp_kernel,
step_jac_kernel with both row kinds, rew_vjp_kernel with an angle control.

Every launch is made twice, on the `special` inputs and on `plain` ones (an ordinary value in every special environment):
(a) bystanders: every gradient of a non-special environment has the same bits in both launches — a lane on the fast path must not
    see what its wave-mates, or the other environments of its own lane, did. No reference, no tolerance.
(b) the special environments against the float64 twin: fp64 within 1e-8 of each tensor's largest magnitude, fp32 within 32 x the
    forward floor (the existing rules; magnitudes over the special environments only, the floor over the special environments of
    the kind that is judged, so that fp32 `mod` angles do not loosen the bound of `zero`, `turns` and `trig32`); where the
    twin's own gradients of a kind move by more than that under one ulp of the special angles, 16 x that spread instead
    (helpers_cold.bound_of). At |theta| ~ 1e10 an ulp is
    2e-6 rad and 1e-8 is out of reach of any implementation; a wrong quadrant is an error of the gradient's own order and misses
    every one of these bounds.
    step_vjp_kernel runs (a) and (b) on every kind too, on the one-step inputs of the step Jacobians.
(c) `mod` and `quad64` alone, K = 1 under "step": the Jacobian is evaluated at the caller's own angle and nothing wraps it first.
    sincos_lean's former `(int)n` quadrant gave sin and cos of such an angle with the wrong sign or swapped (errors of 2.0,
    tools/sincos_lean_restate.c): an error of the Jacobian's own size.
(d) the closed loop: vmap_sim_ahead_feedback_vjp under the full policy, (a) and (b) on all five gradients, and one gain set for all
    as the deterministic batch sum of the per-environment launch on the same special inputs.
Every case prints its launch name, the bystander verdict and per kind the distance, its bound and the rule that set it."""
import numpy as np
import pytest
import torch

from helpers import make_env, to_state
from helpers_cold import (REV_K, bound_of, by_kind, kinds_for, reverse_cases, reverse_forms, reverse_id, spread_by_kind, twin_reference,
                          uniform_kind)
from helpers_vjp import KINK_CAP, GpuRun, dev, obs_floor

pytestmark = pytest.mark.gpu


def _tensors(ga, gs):
    return [ga] + list(gs)


def _judge(what, ref, dtype, env_name, got_special, got_plain, obs, launch):
    """(a) and (b) of one launch pair -> list of problems. got_*: [grad_actions, grad leaves...] as float64 numpy over all B"""
    mask = ref["built"]["mask"]
    idx, kinds, keep = ref["idx"], ref["kinds"], ref["keep"]
    problems = []
    same = all(np.array_equal(s[~mask], p[~mask]) for s, p in zip(got_special, got_plain))
    moved = any(not np.array_equal(s[mask], p[mask], equal_nan=True) for s, p in zip(got_special, got_plain))
    if not same:
        worst = max(float(np.max(np.abs(s[~mask] - p[~mask]))) for s, p in zip(got_special, got_plain))
        problems.append(f"{what}: bystanders differ between the special and the plain launch by up to {worst:.3e}")
    if not moved:
        problems.append(f"{what}: the special environments give the plain launch's gradients: the special values did not arrive")
    want = _tensors(*ref["want"])
    dist = by_kind([g[idx] for g in got_special], want, kinds, keep if dtype == "float32" else None)
    report = []
    for k, d in dist.items():
        # the existing rules: 1e-8 of each tensor's largest magnitude in fp64, 32 x the forward floor in fp32. The floor is taken over
        # the kept special environments of the kind itself, so that a kind whose forward result is loose (an fp32 `mod` angle)
        # does not set the bound of one whose forward result is tight (`zero`, `turns`). A kind may sit in two or three environments
        # only, whose observations can by chance be closer than one rounding of the format: the floor of a kind is at least fp32's
        # epsilon, and the bound never exceeds the one of all the special environments together.
        sel = kinds == k
        if dtype == "float64":
            base = 1e-8
        else:
            floor = max(obs_floor(obs[idx][sel], ref["obs"][sel], env_name, keep[sel]), float(np.finfo(np.float32).eps))
            base = 32 * min(floor, obs_floor(obs[idx], ref["obs"], env_name, keep))
        bound, rule = bound_of(base, ref["spread"][k])
        report.append(f"{k} {d:.2e} <= {bound:.2e} ({rule})")
        if not (np.isfinite(d) and d <= bound):
            problems.append(f"{what}: {k}: distance {d:.3e} from the twin, bound {bound:.3e} ({rule}; existing bound {base:.3e}, "
                            f"spread {ref['spread'][k]:.3e})")
    if dtype == "float32" and 1.0 - keep.mean() > KINK_CAP:
        problems.append(f"{what}: {1.0 - keep.mean():.4f} of the special environments within the kink margin")
    print(f"cold reverse {what}: {launch}; bystanders {'bit-equal' if same else 'DIFFER'}; " + "; ".join(report))
    return problems


def _sim_pair(env_name, dtype, solver, sem, V, sub, ref):
    tdt = getattr(torch, dtype)
    out = []
    for leaves in (ref["built"]["special"], ref["built"]["plain"]):
        run = GpuRun(env_name, ref["spec"], tdt, solver, sem, leaves, ref["acts"], sub=sub, envs_per_lane=V)
        ga, gs = run.vjp(*ref["groups"])
        assert run.launch == f"sim_ahead_vjp_kernel (V={V})", run.launch
        out.append((_tensors(ga, gs), run.obs.cpu().numpy(), run.launch))
    return out


@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_trajectory_gradients_with_special_initial_angles(case):
    """vmap_sim_ahead_vjp under both semantics at V = 1 and the wide form, substeps 1 and 2: (a) and (b)"""
    env_name, deadtime, solver, dtype = case
    uniform = uniform_kind(case, kinds_for(env_name, dtype, reverse=True))
    problems = []
    for sem, V, sub in reverse_forms(env_name, dtype, solver):
        ref = twin_reference(env_name, deadtime, solver, sem, dtype, V, sub, uniform=uniform)
        (special, obs, launch), (plain, _, _) = _sim_pair(env_name, dtype, solver, sem, V, sub, ref)
        problems += _judge(f"{reverse_id(case)} {sem} V={V} substeps={sub} K={REV_K} uniform={uniform}", ref, dtype, env_name, special, plain,
                           obs, launch)
    assert not problems, "\n".join(problems)


def _huge_kinds(dtype):
    return ["mod", "quad64"] if dtype == "float64" else ["mod"]


@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_one_step_at_the_callers_own_huge_angle(case):
    """(c): `mod` and `quad64` alone with K = 1 under "step", through the trajectory kernel and through vmap_step_vjp (the same
    cotangents: the new observation and the new state)"""
    env_name, deadtime, solver, dtype = case
    kinds = _huge_kinds(dtype)
    uniform = kinds[reverse_cases().index(case) % len(kinds)]
    problems = []
    ref = twin_reference(env_name, deadtime, solver, "step", dtype, 1, 1, K=1, uniform=uniform, kinds=kinds)
    (special, obs, launch), (plain, _, _) = _sim_pair(env_name, dtype, solver, "step", 1, 1, ref)
    problems += _judge(f"{reverse_id(case)} step K=1 uniform={uniform} (trajectory kernel)", ref, dtype, env_name, special, plain, obs, launch)
    # the reverse-mode step kernel on the same inputs
    ref = twin_reference(env_name, deadtime, solver, "step", dtype, 1, 1, K=1, uniform=uniform, kinds=kinds, last_only=True)
    problems += _step_vjp_pair(f"{reverse_id(case)} step K=1 uniform={uniform} (step kernel)", ref, env_name, solver, dtype)
    assert not problems, "\n".join(problems)


def _step_vjp_pair(what, ref, env_name, solver, dtype):
    """vmap_step_vjp on the special and on the plain initial states of a K = 1, last_only reference (the cotangents of one step:
    the new observation and the new state) -> _judge's problems"""
    tdt = getattr(torch, dtype)
    g_obs, _, g_last = ref["groups"]
    got = []
    for leaves in (ref["built"]["special"], ref["built"]["plain"]):
        env, _, _, _ = make_env(env_name, ref["acts"].shape[0], tdt, solver, spec=ref["spec"])
        state, action = to_state(env, leaves), dev(ref["acts"][:, 0], env)
        o, new_state = env.vmap_step(state, action)
        ga, gs = env.vmap_step_vjp(state, action, new_state, dev(g_obs[:, -1], env), [dev(g, env) for g in g_last])
        torch.cuda.synchronize()
        launch = env.last_step_vjp_launch
        assert launch == "step_vjp_kernel (V=1)", launch
        f64 = lambda t: t.cpu().numpy().astype(np.float64)
        got.append(([f64(ga)[:, None, :]] + [f64(getattr(gs, n)) for n in env.STATE_FIELDS], f64(o)[:, None, :]))
    # the forward floor of the step: the new observation row against the twin's
    ref = dict(ref, obs=ref["obs"][:, 1:2])
    return _judge(what, ref, dtype, env_name, got[0][0], got[1][0], got[0][1], launch)


@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_step_gradients_with_special_angles(case):
    """vmap_step_vjp at states that hold every reverse kind (`turns`, `trig32`, `mod`, `quad64` in fp64, `zero`), mixed and uniform
    waves: (a) and (b) on the inputs of the step Jacobians below. In fp32 this is where step_vjp_kernel's sincos_lib path (a `trig32`
    angle among fast lanes) meets the twin; the `mod` comparison alone asserts little there beyond (a)."""
    env_name, deadtime, solver, dtype = case
    uniform = uniform_kind(case, kinds_for(env_name, dtype, reverse=True), shift=1)
    ref = twin_reference(env_name, deadtime, solver, "step", dtype, 1, 1, K=1, uniform=uniform, last_only=True)
    problems = _step_vjp_pair(f"{reverse_id(case)} step_vjp every kind uniform={uniform}", ref, env_name, solver, dtype)
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------- parameter gradients
def _angle_written(built, env_name):
    from helpers import ANGLE_STATES

    w = built["written"].copy()
    w[[j for j in range(w.shape[0]) if j not in ANGLE_STATES.get(env_name, [])]] = False
    return w


@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_per_environment_parameter_gradients_with_special_initial_angles(case):
    """vmap_sim_ahead_vjp(param_grads="per_env"), the PGRAD form, V = 1: the per-environment gradients w.r.t. the static parameters
    against helpers_vjp_params.ParamTwin on the special environments, the semantics taking turns over the cases"""
    from helpers_cold import one_ulp
    from helpers_vjp_params import ParamTwin, gpu_param_vjp

    env_name, deadtime, solver, dtype = case
    tdt = getattr(torch, dtype)
    sem = ("ahead", "step")[reverse_cases().index(case) % 2]
    uniform = uniform_kind(case, kinds_for(env_name, dtype, reverse=True), shift=2)
    ref = twin_reference(env_name, deadtime, solver, sem, dtype, 1, 1, uniform=uniform)
    spec, built, acts, idx, grp = ref["spec"], ref["built"], ref["acts"], ref["idx"], ref["groups"]
    sub_grp = (grp[0][idx], [g[idx] for g in grp[1]], [g[idx] for g in grp[2]])

    def twin(leaves):
        tw = ParamTwin(env_name, spec, solver, sem, [v[idx].astype(np.float64) for v in leaves], acts[idx].astype(np.float64), spec["tau"])
        g = tw.grads(sub_grp)
        return [g[k] for k in tw.names], tw.names

    want, names = twin(built["special"])
    angles = _angle_written(built, env_name)
    spread = spread_by_kind(twin(one_ulp(built["special"], angles, +1))[0], twin(one_ulp(built["special"], angles, -1))[0], want, ref["kinds"],
                        ref["keep"])
    got = []
    for leaves in (built["special"], built["plain"]):
        run = GpuRun(env_name, spec, tdt, solver, sem, leaves, acts, envs_per_lane=1)
        _, _, gp = gpu_param_vjp(run, grp)
        assert run.launch == "sim_ahead_vjp_kernel (V=1, PGRAD)", run.launch
        got.append(([gp[k] for k in names], run.obs.cpu().numpy(), run.launch))
    ref = dict(ref, want=(want[0], want[1:]), spread=spread)
    problems = _judge(f"{reverse_id(case)} {sem} per_env parameter gradients uniform={uniform}", ref, dtype, env_name, got[0][0], got[1][0],
                      got[0][1], got[0][2])
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------- step Jacobians
@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_step_jacobians_with_special_angles(case):
    """vmap_linearize, state rows and observation rows, at states that hold every reverse kind: A = d row / d state and
    Bu = d row / d action against the twin's (one-hot cotangents through one "step" twin step on the special environments)"""
    from helpers_cold import one_ulp
    from helpers_vjp import Twin, twin_grads

    env_name, deadtime, solver, dtype = case
    tdt = getattr(torch, dtype)
    uniform = uniform_kind(case, kinds_for(env_name, dtype, reverse=True), shift=1)
    ref = twin_reference(env_name, deadtime, solver, "step", dtype, 1, 1, K=1, uniform=uniform, last_only=True)
    spec, built, acts, idx = ref["spec"], ref["built"], ref["acts"], ref["idx"]
    S, n = len(built["special"]), idx.size
    O = ref["obs"].shape[-1]

    def twin(leaves):
        """-> {"state": [A [n, S, S], Bu [n, S, A]], "obs": [A [n, O, S], Bu [n, O, A]]}"""
        out = {}
        for kind, R in (("state", S), ("obs", O)):
            groups = []
            for r in range(R):
                if kind == "state":
                    groups.append((None, None, [np.ones(n) if j == r else None for j in range(S)]))
                else:
                    e = np.zeros((n, 2, O))
                    e[:, 1, r] = 1.0
                    groups.append((e, None, None))
            rows, _, _ = twin_grads(Twin(env_name, spec, solver, "step"), [v[idx].astype(np.float64) for v in leaves], acts[idx].astype(np.float64),
                                    spec["tau"], 1, groups, O)
            out[kind] = [np.stack([np.stack(gs, axis=-1) for _, gs in rows], axis=1), np.stack([ga[:, 0] for ga, _ in rows], axis=1)]
        return out

    want = twin(built["special"])
    angles = _angle_written(built, env_name)
    up, down = twin(one_ulp(built["special"], angles, +1)), twin(one_ulp(built["special"], angles, -1))
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    problems = []
    got = {}
    for which, leaves in (("special", built["special"]), ("plain", built["plain"])):
        env, _, _, _ = make_env(env_name, acts.shape[0], tdt, solver, spec=spec)
        state, action = to_state(env, leaves), dev(acts[:, 0], env)
        o, new_state = env.vmap_step(state, action)
        for kind in ("state", "obs"):
            A, Bu = env.vmap_linearize(state, action, new_state, rows=kind)
            torch.cuda.synchronize()
            got[which, kind] = ([f64(A), f64(Bu)], f64(o)[:, None, :], env.last_linearize_launch)
    names = {"state": "step_jac_kernel (V=1, state rows)", "obs": "step_jac_kernel (V=1, observation rows)"}
    for kind in ("state", "obs"):
        special, obs, launch = got["special", kind]
        assert launch == names[kind], launch
        r = dict(ref, want=(want[kind][0], want[kind][1:]), spread=spread_by_kind(up[kind], down[kind], want[kind], ref["kinds"], ref["keep"]),
                 obs=ref["obs"][:, 1:2])
        problems += _judge(f"{reverse_id(case)} linearize rows={kind} uniform={uniform}", r, dtype, env_name, special, got["plain", kind][0], obs, launch)
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------- the reward's backward
REWARD_CASES = [(e, d) for e in ("pendulum", "cartpole", "acrobot") for d in ("float32", "float64")]


@pytest.mark.parametrize("env_name,dtype", REWARD_CASES)
def test_reward_backward_with_an_angle_control_at_special_angles(env_name, dtype):
    """vmap_reward_vjp (the backward of vmap_generate_rew_trunc_term_ahead) with an angle among the controlled fields: the stored
    angle rows hold the angle kinds, the angle's reference a `turns` or `trig32` value. Reference: torch.autograd over
    helpers_step_vjp.reward64 in float64 (a central difference cannot resolve an angle whose ulp exceeds its step). Bounds: those of
    tests/test_gpu_reward_vjp.py (1e-7 in fp64, 1e-5 in fp32, of each leaf's largest magnitude), or 16 x the reference's own spread."""
    from helpers import ANGLE_STATES, spec_of
    from helpers_cold import build, special_references
    from helpers_reward_vjp import make_states, reward_inputs, tensor, wide_b
    from helpers_step_vjp import CONTROL, reward64

    tdt = getattr(torch, dtype)
    elem = np.dtype(dtype).itemsize
    V, B, rows = 16 // elem, wide_b(elem), 3
    control = CONTROL[env_name]
    spec = spec_of(env_name)
    base = reward_inputs(env_name, control, B, rows, elem)
    kinds = [k for k in kinds_for(env_name, dtype, reverse=True) if k != "zero"]
    built = build(env_name, spec, dtype, B, V, kinds[REWARD_CASES.index((env_name, dtype)) % len(kinds)], seed=5, reverse=True,
                  plain=[leaf[:, 0] for leaf in base["leaves"]], kinds=kinds)
    mask, idx = built["mask"], np.flatnonzero(built["mask"])
    names = list(control)
    refs = special_references([base["refs"][n] for n in names], names, env_name, mask, dtype, seed=5)
    plain = dict(leaves=[np.array(leaf) for leaf in base["leaves"]], refs={n: np.array(base["refs"][n]) for n in names}, g=np.array(base["g"]))
    special = dict(leaves=[np.array(leaf) for leaf in base["leaves"]], refs={n: r.astype(np.float64) for n, r in zip(names, refs)}, g=plain["g"])
    for j in ANGLE_STATES[env_name]:
        w = built["written"][j]
        special["leaves"][j][w] = built["special"][j][w].astype(np.float64)[:, None]

    def twin(leaves):
        lv = [torch.tensor(np.asarray(v[idx], dtype=np.float64), requires_grad=True) for v in leaves]
        total = torch.zeros((), dtype=torch.float64)
        for r in range(1, rows):
            rew = reward64(env_name, spec, control, [v[:, r] for v in lv], {n: special["refs"][n][idx] for n in names})
            total = total + (rew * torch.as_tensor(special["g"][idx, r - 1])).sum()
        gr = torch.autograd.grad(total, lv, allow_unused=True)
        return [np.zeros((idx.size, rows)) if g is None else g.numpy() for g in gr]

    want = twin(special["leaves"])
    moved = lambda s: [np.nextafter(v.astype(dtype), np.asarray(s * np.inf, dtype=dtype)).astype(np.float64) if j in ANGLE_STATES[env_name]
                       else v for j, v in enumerate(special["leaves"])]
    spread = spread_by_kind(twin(moved(+1)), twin(moved(-1)), want, built["kind"][idx])
    got = {}
    for which, data in (("special", special), ("plain", plain)):
        env, _, _, _ = make_env(env_name, B, tdt, control_state=names)
        gs = env.vmap_reward_vjp(make_states(env, data), tensor(data["g"], env)[..., None])
        torch.cuda.synchronize()
        launch = env.last_reward_vjp_launch
        got[which] = [np.zeros((B, rows)) if getattr(gs, n) is None else getattr(gs, n).cpu().numpy().astype(np.float64) for n in env.STATE_FIELDS]
    assert launch == f"rew_vjp_kernel (V={V})", launch
    same = all(np.array_equal(s[~mask], p[~mask]) for s, p in zip(got["special"], got["plain"]))
    dist = by_kind([g[idx] for g in got["special"]], want, built["kind"][idx])
    existing = 1e-7 if dtype == "float64" else 1e-5
    report, problems = [], []
    for k, d in dist.items():
        bound, rule = bound_of(existing, spread[k])
        report.append(f"{k} {d:.2e} <= {bound:.2e} ({rule})")
        if not d <= bound:
            problems.append(f"{k}: distance {d:.3e}, bound {bound:.3e} ({rule})")
    print(f"cold reverse reward {env_name} {dtype} control={control}: {launch}; bystanders {'bit-equal' if same else 'DIFFER'}; " + "; ".join(report))
    assert same, "bystanders differ between the special and the plain launch"
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------- the closed loop's reverse mode
@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_closed_loop_gradients_with_special_initial_angles(case):
    """vmap_sim_ahead_feedback_vjp (feedback_z_rows_kernel, sim_feedback_vjp_kernel, feedback_gain_grad_kernel) with every reverse kind in
    the initial state: B = 326, K = 3, substeps 1 and 2 (PMSM: 1), the full policy (per-environment gains, integral action,
    feedforward, clip), all five cotangents. (a) bystanders: grad_state0, grad_gain, grad_integral_gain, grad_ff and grad_z0 of every
    non-special environment have the same bits in the `special` and the `plain` launch; (b) the special environments against the
    float64 closed-loop twin under _judge's rules as they are (1e-8 in fp64, 32 x the forward floor in fp32, per kind, or 16 x the
    twin's own spread under one ulp of the special angles: helpers_cold.feedback_twin_reference). The fp32 forward floor is taken
    over the rows the launch computed (1 .. N). With row 0 in it — the caller's own unwrapped angle, normalised: 3e7 in the `mod`
    environments — obs_floor's scale is that number, the floor of "all special environments" becomes 5.3e-8 (the rounding of 3e7,
    no forward error at all), and a `zero` environment at omega = its lower bound (distance 1.7e-6 .. 3.3e-6 in three cases, below
    32 fp32 epsilons) was held to 1.69e-6 by the angle of another environment.
    One gain set for all, once per case: the bystander rule cannot apply to a sum over the batch; instead the sum is, bit for bit,
    excenv_param_grad_sum of the per-environment launch on the same special inputs (and every other gradient that launch's)."""
    from helpers_cold import feedback_reverse_subs, feedback_twin_reference
    from test_gpu_feedback_vjp import assert_batch_sum_identity, explicit, forward

    env_name, deadtime, solver, dtype = case
    tdt = getattr(torch, dtype)
    uniform = uniform_kind(case, kinds_for(env_name, dtype, reverse=True), shift=3)
    flat = lambda g: list(g["state0"]) + [g["gain"], g["igain"], g["ff"], g["z0"]]
    problems = []
    for n, sub in enumerate(feedback_reverse_subs(env_name)):
        ref = feedback_twin_reference(env_name, deadtime, solver, dtype, sub, uniform)
        spec, built, inp, group = ref["spec"], ref["built"], ref["inp"], ref["group"]
        B = built["mask"].shape[0]
        got = {}
        for which in ("special", "plain"):
            data = dict(inp, st=[v.astype(np.float64) for v in built[which]])
            env, _, _, _ = make_env(env_name, B, tdt, solver, spec=spec)
            run = forward(env, data, REV_K, sub, spec["tau"])
            got[which] = (flat(explicit(run, group)), run["obs"].cpu().numpy().astype(np.float64))
            assert env.last_feedback_vjp_cotangents == dict(obs=True, states=[True] * env.physical_state_dim,
                                                            last_state=[True] * env.physical_state_dim, actions=True, z=True)
            if which == "special" and n == 0:  # one gain set for all, on the special inputs
                one = dict(data, gain=inp["gain"][0], igain=inp["igain"][0])
                run_b = forward(env, one, REV_K, sub, spec["tau"])
                assert_batch_sum_identity(run_b, group, explicit(run_b, group), f"cold reverse {reverse_id(case)} substeps={sub} one gain set for all")
        # the forward floor over the rows the launch computed: row 0 is the caller's own state normalised, an unwrapped angle of 3e7 pi
        # there sets the scale of obs_floor for every kind and says nothing about the forward error (as _step_vjp_pair: the new row)
        problems += _judge(f"{reverse_id(case)} closed loop substeps={sub} K={REV_K} uniform={uniform}", dict(ref, obs=ref["obs"][:, 1:]), dtype,
                           env_name, got["special"][0], got["plain"][0], got["special"][1][:, 1:], "sim_feedback_vjp_kernel")
    assert not problems, "\n".join(problems)
