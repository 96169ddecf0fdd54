"""The forward kernels off the fast paths (``-m gpu``): unwrapped and huge angles, zero / huge / NaN / inf leaves, in mixed and
uniform waves of a real kernel.

tests/helpers_cold.py defines the special values per kind and the lane pattern (tests/test_cold_paths_host.py checks both without a
GPU). Every case launches one kernel form twice through the C entry points (the launchers of tests/test_gpu_guard_forward.py on
ordinary tensors): on the `special` inputs and on `plain` ones, the same arrays with an ordinary value in every special environment.

(a) Bystanders. Every output (observations, state rows, last state, reward, flags) of every environment that is not special is
    torch.equal between the two launches. A lane on the fast path must not see what its wave-mates, or the other environments of its
    own lane at two or four per lane, did. No reference, no tolerance.
(b) The special environments against the CPU oracle on the same inputs with the bounds of tests/test_gpu_parity.py::_tol: identical
    bits (NaN included) for mass-spring-damper and tank, 1e-9 (fp64) / 1e-5 (fp32) for the rest, angles on the circle; NaN and inf at
    the oracle's positions. Where a case misses that bound, the oracle's own spread under one ulp of the special leaves is measured
    and 16 x that spread is the bound (helpers_cold.bound_of; both figures are printed). Distance and spread are taken per kind, so
    that a kind whose spread is large does not set the bound of the others. The reward and the flags are judged on the state rows
    the launch itself wrote, as tests/test_gpu_gym.py judges them.
Every launch's name (excenv_last_launch) is asserted. Every case prints it with the bystander verdict and the distance, its bound
and the rule that set the bound.

sim_ahead_emr_kernel redoes a block of rows with the guarded M::observe when observe_defer reports `bad` (kernels_emr.hpp). That the
block runs is known from the data, not only from the guard's code: for an `inf` leaf the unguarded quotient is NaN (fastq: q = inf * y,
then the residual fma(-b, inf, inf) = NaN), the plain division gives inf. The oracle's observation of such an environment holds inf,
and (b) demands inf at the same positions — only the redone block can deliver it. The case asserts that the oracle's rows do hold inf.

The lane pattern is built for lane = env // V, wave = lane // 64, which every form here follows but sim_ahead_emr_kernel: its waves
interleave (env = env0 + P * lane, P = helpers_guard.emr_period, up to 32 in these cases), so in the emr cases every wave that holds a special environment is
mixed and none is uniform (fp32: all 32 waves mixed; fp64: 9 or 17 mixed, 15 clean); their printed wave summary comes from that
kernel's own map (helpers_cold.wave_summary(period=P)).

The saturated PMSM gets finite currents far outside its tables and NaN only (helpers_cold.SATURATED_KINDS). K <= 3 except where a form
needs whole 16-byte action rows (row-major actions fused, the register ring: K = 4 in fp32)."""
import numpy as np
import pytest
import torch

import oracle
from helpers import ANGLE_OBS, ANGLE_STATES, TRIG_FREE
from helpers_cold import (bound_of, build, finite_distance, kinds_for, nonfinite_equal, one_ulp, special_references,
                          wave_summary)
from helpers_forms import MODEL_CASES, SEM_ID
from helpers_guard import VMAX, Plain, _case, _lean_name, emr_period, guard_inputs
from test_gpu_guard_forward import ctx_of, run_rew, run_sim, run_step
from test_gpu_parity import _tol

pytestmark = pytest.mark.gpu

B = 1304           # helpers_forms.B
B_WAVES = 1280     # row-major actions fused: whole waves at every lane width (sim_plan.hpp reads_row_major_actions)
SIX = ["pendulum", "mass_spring_damper", "cartpole", "acrobot", "fluid_tank", "pmsm_deadtime1"]
SOLVER_OF = {"pendulum": "tsit5", "mass_spring_damper": "euler", "cartpole": "euler", "acrobot": "tsit5", "fluid_tank": "tsit5",
             "pmsm_deadtime1": "euler", "pmsm_deadtime0": "tsit5"}


def _other(solver):
    return "tsit5" if solver == "euler" else "euler"


def forward_cases():
    """[(id, case dict of helpers_guard._case + `uniform`: the kind wave 3 holds, by name or as a running number into the kinds
    that apply to the model)]"""
    out = []

    def add(name, n, **kw):
        out.append((name, dict(_case(kw.pop("kind", "sim"), **kw), uniform=n)))

    n = 0
    for m in SIX + ["pmsm_deadtime0"]:
        for d in ("float32", "float64"):
            A = 2 if "pmsm" in m else 1
            elem = 4 if d == "float32" else 8
            # step_kernel at every lane width and the general form
            for V in (1, 2, 4):
                if V <= VMAX[d]:
                    n += 1
                    add(f"step-V{V}-{m}-{d}", n, kind="step", model=m, dtype=d, B=B, epl=V, solver=SOLVER_OF[m] if V > 1 else _other(SOLVER_OF[m]),
                        expect=f"step_kernel (V={V})")
            n += 1
            add(f"step-general-{m}-{d}", n, kind="step", model=m, dtype=d, B=B, controls=1, gym=True, solver=SOLVER_OF[m],
                expect="step_kernel (general)")
            # sim_ahead_kernel lean at one per lane and the widest, under the three semantics
            for V in (1, VMAX[d]):
                for sem in ("step", "ahead", "ahead_accumulated_t"):
                    n += 1
                    add(f"lean-V{V}-{sem}-{m}-{d}", n, model=m, dtype=d, B=B, K=3, sem=sem, epl=V, solver=SOLVER_OF[m] if sem != "ahead" else
                        _other(SOLVER_OF[m]), expect=_lean_name(V, sem))
            if m == "pmsm_deadtime0":
                continue
            n += 1
            add(f"general-{m}-{d}", n, model=m, dtype=d, B=B, K=3, per_env=True, sem="ahead", solver=SOLVER_OF[m], expect="sim_ahead_kernel (general)")
            n += 1
            add(f"em-{m}-{d}", n, model=m, dtype=d, B=B, K=3 if (B * 3 * A * elem) % 16 == 0 else 2, a="env", t="env", emm=2, sem="step",
                solver=_other(SOLVER_OF[m]), expect="sim_ahead_em_kernel")
            # the lean gym form: an angle among the controlled fields where the model has one
            controls = {"cartpole": 3}.get(m, 1)
            n += 1
            add(f"lean_gym-{m}-{d}", n, model=m, dtype=d, B=B, K=3, controls=controls, gym=True, epl=VMAX[d], solver="euler",
                expect="sim_ahead_kernel (lean, gym outputs)")
            n += 1
            add(f"rew-{m}-{d}", n, kind="rew", model=m, dtype=d, B=B, rows=3, controls=controls, out_lane=True, in_lane=True, vary=False)
    n = 0
    for m in ("pendulum", "cartpole", "mass_spring_damper"):  # substeps = 3
        for d in ("float32", "float64"):
            n += 1
            add(f"substeps3-{m}-{d}", n, model=m, dtype=d, B=B, K=2, sub=3, sem="ahead", epl=VMAX[d], solver="tsit5", expect=_lean_name(VMAX[d], "ahead"))
    for m in ("pendulum", "cartpole", "pmsm_deadtime1"):
        A = 2 if "pmsm" in m else 1
        for d in ("float32", "float64"):
            elem = 4 if d == "float32" else 8
            K = max(1, 16 // (A * elem))  # whole 16-byte action rows
            n += 1
            add(f"aem-{m}-{d}", n, model=m, dtype=d, B=B_WAVES, K=K, a="env", epl=VMAX[d], sem="ahead", solver=SOLVER_OF[m],
                expect="sim_ahead_kernel (row-major actions fused)")
            if m == "pmsm_deadtime1" and d == "float64":
                continue  # models.hpp observe_defer_ok: no deferred block for PMSM in fp64
            for sem in ("step", "ahead"):
                add(f"emr-{sem}-{m}-{d}", "inf" if sem == "step" else "zero", model=m, dtype=d, B=B, K=K, a="env", t="env", emm=3, sem=sem, solver=SOLVER_OF[m],
                    expect="sim_ahead_emr_kernel", emr=True)
    for d in ("float32", "float64"):  # the saturated PMSM, tables in LDS
        for k, solver in enumerate(("euler", "rk4")):
            n += 1
            add(f"saturated-{solver}-{d}", n, model="pmsm_saturated_lds", solver=solver, dtype=d, B=B, K=2, sem=("step", "ahead")[k], epl=1,
                expect=_lean_name(1, ("step", "ahead")[k]))
        n += 1
        add(f"saturated-step-{d}", n, kind="step", model="pmsm_saturated_lds", dtype=d, B=B, epl=1, expect="step_kernel (V=1)")
    # the 1024-thread lean gym form exists from B / V >= 2^18 on, so this one case is far larger than the others (B = 2^20 + 260,
    # K = 2, still well under a second), judged on the special environments like the rest. Pendulum fp32 is the only model with an
    # angle that has the form: sim_plan.hpp sim_wide_gym_ok excludes the fp64 pendulum, and no other model with an angle is sim_wide_ok.
    add("lean_gym_1024-pendulum-float32", 1, model="pendulum", dtype="float32", B=(1 << 20) + 260, K=2, controls=1, gym=True, epl=4,
        expect="sim_ahead_kernel (lean, gym outputs, 1024 threads)")
    return out


CASES = forward_cases()
RUN = {"sim": run_sim, "step": run_step, "rew": run_rew}


def _inputs(ctx, c):
    """-> special inputs, plain inputs, build() record"""
    saturated = MODEL_CASES[c["model"]][2] is not None
    kinds = kinds_for(ctx.env_name, c["dtype"], saturated=saturated)
    uniform = c["uniform"] if isinstance(c["uniform"], str) else kinds[c["uniform"] % len(kinds)]
    V = max(1, c["epl"]) if c["kind"] != "rew" else 1
    rows = c.get("rows", 0)
    plain = guard_inputs(ctx.env_name, ctx.spec, c["dtype"], c["B"], 1 if c["kind"] == "step" else c["K"], ctx.names, rows=rows)
    built = build(ctx.env_name, ctx.spec, c["dtype"], c["B"], V, uniform, seed=7, saturated=saturated, plain=plain["st"])
    special = dict(plain, st=built["special"])
    if ctx.names:
        special["refs"] = special_references(plain["refs"], ctx.names, ctx.env_name, built["mask"], c["dtype"], seed=7)
    if rows:  # a stored trajectory: the special leaves in every saved row
        special["leaves"] = [leaf.copy() for leaf in plain["leaves"]]
        for j in range(ctx.S):
            w = built["written"][j]
            special["leaves"][j][w] = built["special"][j][w][:, None]
    return special, plain, built


def _oracle_outputs(ctx, c, inp, idx):
    """The oracle's outputs of the case on the environments idx (all of them for per-environment properties) -> dict like the
    launchers' `out`, env-major, without the gym outputs (those are judged on the launch's own state rows)"""
    npdt = np.dtype(c["dtype"]).type
    if c["per_env"]:
        props, sel = ctx.oprops, slice(None)
    else:
        lut = None
        if MODEL_CASES[c["model"]][2] is not None:
            from exciting_environments_amd import prepare_pmsm_lut
            from helpers_forms import saturated_tables

            lut = prepare_pmsm_lut(saturated_tables(c["model"]))
        props, keep = oracle.make_props(ctx.env_name, ctx.spec["params"], ctx.spec["phys_norm"], ctx.spec["act_norm"], npdt, idx.size, pmsm_lut=lut)
        sel = idx
    st = [v[sel] for v in inp["st"]]
    control = [(n, r[sel]) for n, r in zip(ctx.names, inp["refs"])]
    tau = ctx.spec["tau"]
    out = {}
    if c["kind"] == "step":
        obs, new = oracle.step(ctx.env_name, c["solver"], st, inp["acts"][sel, 0], props, tau, control=control)
        out["obs"] = obs
        out.update({f"state_out[{j}]": v for j, v in enumerate(new)})
    else:
        obs, states, last = oracle.sim_ahead(ctx.env_name, c["solver"], st, inp["acts"][sel], props, tau / c["sub"], env_tau=tau, substeps=c["sub"],
                                             semantics=SEM_ID[c["sem"]], control=control)
        out["obs"] = obs
        out.update({f"state_traj[{j}]": v for j, v in enumerate(states)})
        out.update({f"last_state[{j}]": v for j, v in enumerate(last)})
    if c["per_env"]:
        out = {k: v[idx] for k, v in out.items()}
    return out


def _normalised(ctx, j, x, idx):
    """A state leaf in observation units (float64), so that the bound of the observations applies to it"""
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (ctx.props_B,))[idx] for v in ctx.spec["phys_norm"][oracle.STATE_FIELDS[ctx.env_name][j]])
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        lo, hi = lo[:, None], hi[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return ((x - lo) / (hi - lo) * 2 - 1)[..., None]


def _distance(ctx, c, got, want, idx):
    """-> (largest distance of the float outputs in observation units, names whose NaN / inf positions differ, names that differ in
    bits — the trig-free rule)"""
    worst, nonfinite, bits = 0.0, [], []
    for name, w in want.items():
        g = got[name]
        if ctx.env_name in TRIG_FREE and not np.array_equal(g, w, equal_nan=True):
            bits.append(name)
        if not nonfinite_equal(g, w):
            nonfinite.append(name)
        if name == "obs":
            worst = max(worst, finite_distance(g, w, ANGLE_OBS.get(ctx.env_name, [])))
        else:
            j = int(name[name.index("[") + 1:-1])
            worst = max(worst, finite_distance(_normalised(ctx, j, g, idx), _normalised(ctx, j, w, idx), [0] if j in ANGLE_STATES.get(ctx.env_name, []) else []))
    return worst, nonfinite, bits


def _gym_problems(ctx, c, inp, host, idx):
    """Reward and flags of the special environments against the oracle's on the state rows this launch wrote"""
    npdt = np.dtype(c["dtype"]).type
    props, keep = (ctx.oprops, None) if c["per_env"] else oracle.make_props(ctx.env_name, ctx.spec["params"], ctx.spec["phys_norm"],
                                                                           ctx.spec["act_norm"], npdt, idx.size)
    control = [(n, r[idx]) for n, r in zip(ctx.names, inp["refs"])]
    tol = max(_tol(ctx.env_name, ctx.dtype)[0], 0.0)
    bad = []
    if c["kind"] == "step":
        own = [np.ascontiguousarray(host[f"state_out[{j}]"][idx])[:, None].repeat(2, axis=1) for j in range(ctx.S)]
        rew, trunc, term = oracle.rew_trunc_term_ahead(ctx.env_name, own, props, control=control)
        r, te, tr = host["reward"][idx][:, None], host["terminated"][idx][:, None], host["truncated"][idx]
        rew, term, trunc = rew[..., 0], term[..., 0], trunc[:, 1]
    else:
        if c["kind"] == "rew":
            own = [np.ascontiguousarray(leaf[idx]) for leaf in inp["leaves"]]
        else:
            own = [np.ascontiguousarray(host[f"state_traj[{j}]"][idx]) for j in range(ctx.S)]
        rew, trunc, term = oracle.rew_trunc_term_ahead(ctx.env_name, own, props, control=control)
        r, te, tr = host["reward"][idx], host["terminated"][idx], host["truncated"][idx]
        rew, term = rew[..., 0], term[..., 0]
    d = finite_distance(r, rew)
    if not nonfinite_equal(r, rew):
        bad.append("reward: NaN / inf positions differ from the oracle's")
    if (tol == 0.0 and not np.array_equal(r, rew, equal_nan=True)) or d > tol:
        bad.append(f"reward: distance {d:.3e} from the oracle on the launch's own state rows, bound {tol:.1e}")
    if not np.array_equal(te, term):
        bad.append("terminated differs from the oracle's")
    if not np.array_equal(tr, trunc):
        bad.append("truncated differs from the oracle's")
    return bad, d


def _one_case(name, c):
    ctx = ctx_of(c)
    ctx.props_B = c["B"]
    special, plain, built = _inputs(ctx, c)
    mask, idx = built["mask"], np.flatnonzero(built["mask"])
    launch_s, out_s = RUN[c["kind"]](ctx, c, special, Plain())
    torch.cuda.synchronize()
    launch_p, out_p = RUN[c["kind"]](ctx, c, plain, Plain())
    torch.cuda.synchronize()
    problems = []
    if c["expect"] is not None and not (launch_s == launch_p == c["expect"]):
        problems.append(f"launched {launch_s!r} / {launch_p!r}, the case was built to reach {c['expect']!r}")
    # (a) bystanders
    calm = torch.as_tensor(~mask, device=out_s["obs" if "obs" in out_s else "truncated"].device)
    differ = [n for n in out_s if not torch.equal(out_s[n][calm], out_p[n][calm])]
    if differ:
        problems.append(f"bystanders: {differ} differ between the special and the plain launch")
    host = {n: t.cpu().numpy() for n, t in out_s.items()}
    # (b) the special environments against the oracle
    report = ""
    if c["kind"] != "rew":
        want = _oracle_outputs(ctx, c, special, idx)
        got = {n: host[n][idx] for n in want}
        if c.get("emr"):  # the evidence that the redone block ran (module text)
            infs = built["kind"][idx] == "inf"  # (one of the single slots where wave 3 holds another kind)
            assert infs.any() and np.isinf(want["obs"][infs]).any(), "no inf in the oracle's observations of the inf environments"
        _, nonfinite, bits = _distance(ctx, c, got, want, idx)
        tol = _tol(ctx.env_name, ctx.dtype)[0]
        if nonfinite:
            problems.append(f"special environments: NaN / inf positions of {nonfinite} differ from the oracle's")
        if tol == 0.0 and bits:
            problems.append(f"special environments: {bits} differ from the oracle's bits")
        # distances and bounds per kind, so that the spread of one kind (an fp32 `mod` angle moves by radians under one ulp) does
        # not become the bound of the others
        of = lambda out, sel: {n: v[sel] for n, v in out.items()}
        up = down = None
        parts = []
        for k in sorted(set(built["kind"][idx])):
            sel = built["kind"][idx] == k
            d = _distance(ctx, c, of(got, sel), of(want, sel), idx[sel])[0]
            bound, rule = tol, "existing bound"
            if tol > 0.0 and d > tol:  # the oracle's own spread under one ulp of the special leaves
                if up is None:
                    up = _oracle_outputs(ctx, c, dict(special, st=one_ulp(special["st"], built["written"], +1)), idx)
                    down = _oracle_outputs(ctx, c, dict(special, st=one_ulp(special["st"], built["written"], -1)), idx)
                spread = _distance(ctx, c, of(up, sel), of(down, sel), idx[sel])[0]
                bound, rule = bound_of(tol, spread)
                rule += f" (spread {spread:.3e})"
                if d > bound:
                    problems.append(f"special environments: {k}: distance {d:.3e} from the oracle, bound {bound:.3e} ({rule})")
            parts.append(f"{k} {d:.3e} <= {bound:.3e} ({rule})")
        report = "special environments " + ", ".join(parts)
    if c["gym"] or c["kind"] == "rew":
        bad, d = _gym_problems(ctx, c, special, host, idx)
        problems += bad
        report += f"; reward on own rows {d:.3e}"
    if c.get("emr"):
        # the register ring places env0 + P * lane in a wave (P = emr_period, 32 / 16 in the pendulum cases): where P > 1 the lane
        # pattern, built for lane = env // V, gives it no clean and no uniform wave, only mixed ones. What these cases add is the
        # redone block (module text) and the bystanders of those mixed waves.
        waves = wave_summary(mask, 1, emr_period(ctx.env_name, c["dtype"], c["K"], c["sem"] == "ahead"))
        assert "mixed" in waves, waves
        waves = ", ".join(f"{waves.count(w)} {w}" for w in ("mixed", "clean", "uniform")) + " by the register ring's own lane map"
    else:
        waves = wave_summary(mask, built["V"])
        assert waves[:4] == ["mixed", "mixed", "clean", "uniform"] and waves[-1] != "clean", waves[:4] + waves[-1:]
        waves = f"{waves[:4]}...{waves[-1]}"
    print(f"cold forward {name}: {launch_s}; uniform kind {built['uniform']}, waves {waves}; bystanders "
          f"{'bit-equal' if not differ else 'DIFFER'}; {report}")
    return problems


@pytest.mark.parametrize("name,c", CASES, ids=[n for n, _ in CASES])
def test_special_values_in_mixed_and_uniform_waves(name, c):
    try:
        problems = _one_case(name, c)
    except RuntimeError as e:  # a fault the device reports: nothing more is launched
        if "HIP" not in str(e) and "rc=-3" not in str(e):
            raise
        pytest.exit(f"cold forward {name}: {e}", returncode=3)
    assert not problems, "\n".join(problems)


# ------------------------------------------------------------------------------------------------- the closed loop
FEEDBACK_CASES = [(e, d, s, t) for (e, d), s in zip([("pendulum", None), ("cartpole", None), ("acrobot", None), ("pmsm", 0), ("pmsm", 1)],
                                                    ["tsit5", "euler", "rk4", "euler", "tsit5"]) for t in ("float32", "float64")]


@pytest.mark.parametrize("env_name,deadtime,solver,dtype", FEEDBACK_CASES)
def test_closed_loop_with_special_initial_angles(env_name, deadtime, solver, dtype):
    """sim_feedback_kernel on helpers_feedback.main_case with the angle kinds in the initial state: the three helpers of
    tests/test_gpu_feedback.py as they are (the open-loop kernel on the returned actions bit for bit; every action and the
    integrator within their rounding bounds of the returned observation rows), and the bystanders of (a): observations, actions
    and integrator state of every other environment have the bits of the run on the plain inputs."""
    import helpers_feedback as hf
    from helpers import make_env
    from test_gpu_feedback import check_dynamics, check_policy, closed_loop

    tdt = getattr(torch, dtype)
    spec, inp = hf.main_case(env_name, deadtime)
    kinds = [k for k in kinds_for(env_name, dtype, reverse=True) if k != "zero"]
    uniform = kinds[FEEDBACK_CASES.index((env_name, deadtime, solver, dtype)) % len(kinds)]
    built = build(env_name, spec, dtype, hf.B_MAIN, 1, uniform, seed=72, reverse=True, plain=[np.asarray(v).astype(dtype) for v in inp["st"]],
                  kinds=kinds)
    runs = {}
    for which in ("special", "plain"):
        data = dict(inp, st=[v.astype(np.float64) for v in built[which]])
        env, _, _, _ = make_env(env_name, hf.B_MAIN, tdt, solver, spec=spec)
        run = closed_loop(env, data, hf.K_MAIN, hf.substeps_of(env_name), spec["tau"])
        check_dynamics(run)
        check_policy(run, data)
        runs[which] = run
    calm = torch.as_tensor(~built["mask"], device=runs["special"]["obs"].device)
    same = all(torch.equal(runs["special"][n][calm], runs["plain"][n][calm]) for n in ("obs", "actions", "z"))
    moved = not torch.equal(runs["special"]["obs"][~calm], runs["plain"]["obs"][~calm])
    print(f"cold forward feedback {env_name} deadtime={deadtime} {solver} {dtype}: sim_feedback_kernel; uniform kind {uniform}; bystanders "
          f"{'bit-equal' if same else 'DIFFER'}; dynamics bit-equal to the open-loop launch; policy within its rounding bounds")
    assert same and moved
    assert bool(torch.isfinite(runs["special"]["obs"]).all())


@pytest.mark.parametrize("env_name,deadtime,solver,dtype", FEEDBACK_CASES)
def test_policy_rollout_with_special_initial_angles(env_name, deadtime, solver, dtype):
    """sim_policy_kernel on helpers_policy.main_case (network N1, the activation alternating with the case index) with the angle kinds
    in the initial state: the helpers of tests/test_gpu_policy.py as they are (the open-loop kernel on the returned actions bit for
    bit; ReLU actions bit for bit the contract on the returned observation rows, tanh actions within the forward bound), and the
    bystanders of (a): observations and actions of every other environment have the bits of the run on the plain inputs.
    The launch is 64 wide (policy.hpp POLICY_BLOCK), one wavefront per workgroup, so the lane pattern of special_envs(B, 1) puts the
    uniform special wave into workgroup 3 and mixed waves into workgroups 0 and 1 (and the tail's, workgroup 5); workgroup 2 is clean."""
    import helpers_policy as hp
    from helpers import make_env
    from test_gpu_policy import check_dynamics, check_policy, rollout

    tdt = getattr(torch, dtype)
    n = FEEDBACK_CASES.index((env_name, deadtime, solver, dtype))
    activation = hp.ACTIVATIONS[n % len(hp.ACTIVATIONS)]
    spec, inp = hp.main_case(env_name, deadtime, "N1")
    kinds = [k for k in kinds_for(env_name, dtype, reverse=True) if k != "zero"]
    uniform = kinds[n % len(kinds)]
    built = build(env_name, spec, dtype, hp.B_MAIN, 1, uniform, seed=hp.SEED, reverse=True, plain=[np.asarray(v).astype(dtype) for v in inp["st"]],
                  kinds=kinds)
    waves = wave_summary(built["mask"], 1)
    assert waves[:4] == ["mixed", "mixed", "clean", "uniform"] and waves[-1] == "mixed", waves
    runs = {}
    for which in ("special", "plain"):
        data = dict(inp, st=[v.astype(np.float64) for v in built[which]])
        env, _, _, _ = make_env(env_name, hp.B_MAIN, tdt, solver, spec=spec)
        run = rollout(env, data, activation, hp.K_MAIN, hp.substeps_of(env_name), spec["tau"])
        check_dynamics(run)
        check_policy(run, data)
        runs[which] = run
    calm = torch.as_tensor(~built["mask"], device=runs["special"]["obs"].device)
    same = all(torch.equal(runs["special"][n][calm], runs["plain"][n][calm]) for n in ("obs", "actions"))
    moved = not torch.equal(runs["special"]["obs"][~calm], runs["plain"]["obs"][~calm])
    print(f"cold forward policy {env_name} deadtime={deadtime} {solver} {dtype} {activation}: sim_policy_kernel; uniform kind {uniform}; "
          f"bystanders {'bit-equal' if same else 'DIFFER'}; dynamics bit-equal to the open-loop launch; policy "
          f"{'bit-equal to the exact contract' if activation == 'relu' else 'within its forward bound'}")
    assert same and moved
    assert bool(torch.isfinite(runs["special"]["obs"]).all())
