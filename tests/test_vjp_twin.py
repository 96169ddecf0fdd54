"""The float64 torch twin (tests/helpers_vjp.py) is validated before anything is compared with it: its forward observations
against the fp64 CPU oracle, both semantics, every model and solver, PMSM with dead time 0 and 1 — 64 environments x K = 50,
1e-9 on normalised observations (both sides are fp64 and differ by summation order only; 1e7 x eps leaves room for 50 steps and
the acrobot's amplification). The same file asserts, on the twin's own forward of the GPU tests' inputs, that at most 2 % of the
environments come within the kink margin: the inputs are known to be usable before a GPU is involved."""
import numpy as np
import pytest
import torch

import oracle
from helpers import spec_of
from helpers_vjp import (CASES, DRY_MARGIN, DRY_STEP_FACTOR, KINK_CAP, KINK_MARGIN, SEM, SKEW, SOLVERS, WIDE_CASES, Twin, case_spec,
                         dry_tank_inputs, leaves, skewed_spec, vjp, vjp_inputs, wide_inputs)


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_twin_forward_matches_the_fp64_oracle(env_name, deadtime, solver, semantics):
    B, K = 64, 50
    spec = case_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B, K, seed=3)
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    tau = spec["tau"]
    o_ref, _, _ = oracle.sim_ahead(env_name, solver, st, acts, props, tau, env_tau=tau, semantics=SEM[semantics])
    twin = Twin(env_name, spec, solver, semantics)
    with torch.no_grad():
        obs, _, _ = twin.sim_ahead(leaves(st), torch.as_tensor(acts), tau)
    got, want = obs.numpy(), np.array(o_ref)
    if env_name in ("pendulum", "cartpole", "acrobot"):  # a wrapped angle at +-pi is the same angle: compare on the circle
        from helpers import ANGLE_OBS
        for c in ANGLE_OBS[env_name]:
            d = np.abs(got[..., c] - want[..., c])
            got[..., c] = np.where(np.abs(d - 2.0) < 1e-9, want[..., c], got[..., c])
    err = float(np.max(np.abs(got - want)))
    print(f"{env_name} dead={deadtime} {solver} {semantics}: twin vs oracle max |d obs| = {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("env_name,deadtime", [("mass_spring_damper", None), ("pendulum", None)])
def test_twin_forward_matches_the_oracle_with_substeps(env_name, deadtime):
    B, K, sub = 64, 12, 4
    spec = case_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B, K, seed=4)
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    tau = spec["tau"]
    for semantics in ("ahead", "step"):
        o_ref, _, _ = oracle.sim_ahead(env_name, "rk4", st, acts, props, tau, env_tau=tau, substeps=sub, semantics=SEM[semantics])
        with torch.no_grad():
            obs, _, _ = Twin(env_name, spec, "rk4", semantics).sim_ahead(leaves(st), torch.as_tensor(acts), tau, sub)
        assert float(np.max(np.abs(obs.numpy() - np.array(o_ref)))) <= 1e-9


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_gpu_test_inputs_stay_clear_of_kinks(env_name, deadtime, solver, semantics):
    """The inputs of tests/test_gpu_vjp.py (B = 256, K = 40): the share of environments the fp32 comparison would exclude."""
    B, K = 256, 40
    spec = case_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B, K, seed=11)
    twin = Twin(env_name, spec, solver, semantics)
    with torch.no_grad():
        twin.sim_ahead(leaves(st), torch.as_tensor(acts), spec["tau"])
    kd = twin.kink_distance()
    share = 0.0 if kd is None else float((kd < KINK_MARGIN).double().mean())
    print(f"{env_name} dead={deadtime} {solver} {semantics}: {share:.4f} of the environments within {KINK_MARGIN} of a kink")
    assert share <= KINK_CAP
    if env_name == "pmsm":  # some but not most rows clip: the clamped branch of the transposed clip is exercised, the open one too
        clip = twin.clip_share()
        print(f"pmsm dead={deadtime} {solver} {semantics}: the hexagon clip is active in {clip:.3f} of the action-path evaluations")
        assert 0.01 < clip < 0.5


# ---- the input families of tests/test_gpu_vjp_edges.py: the twin against the oracle, and the shares the GPU tests rely on --------------
def twin_vs_oracle(env_name, spec, solver, semantics, st, acts, step, sub=1):
    """max |d obs| of the twin's forward from the fp64 oracle's (wrapped angles on the circle)"""
    from helpers import ANGLE_OBS

    B = st[0].shape[0]
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    o_ref, _, _ = oracle.sim_ahead(env_name, solver, st, acts, props, step, env_tau=spec["tau"], substeps=sub, semantics=SEM[semantics])
    twin = Twin(env_name, spec, solver, semantics)
    with torch.no_grad():
        obs, _, _ = twin.sim_ahead(leaves(st), torch.as_tensor(acts), step, sub)
    d = np.abs(obs.numpy() - np.array(o_ref))
    for c in ANGLE_OBS.get(env_name, []):
        d[..., c] = np.where(np.abs(d[..., c] - 2.0) < 1e-9, 0.0, d[..., c])
    return float(d.max()), twin


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_twin_forward_matches_the_oracle_at_the_skewed_spec(env_name, deadtime, solver, semantics):
    spec = skewed_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, 64, 50, seed=3)
    err, _ = twin_vs_oracle(env_name, spec, solver, semantics, st, acts, spec["tau"])
    print(f"{env_name} dead={deadtime} {solver} {semantics} skewed: twin vs oracle max |d obs| = {err:.3e}")
    assert err <= 1e-9


def test_skewed_spec_leaves_no_parameter_at_its_default_or_at_one():
    for env_name, deadtime in CASES:
        base, spec = spec_of(env_name), skewed_spec(env_name, deadtime)
        vals = {k: v for k, v in spec["params"].items() if k != "deadtime"}
        assert all(v != 1 and v != base["params"][k] for k, v in vals.items()), env_name
        assert len(set(vals.values())) == len(vals), env_name  # no two equal
        fs = list(SKEW[env_name].values())
        assert len(set(fs)) == len(fs) and all(0.75 <= f <= 0.9 or 1.1 <= f <= 1.35 for f in fs)
        for lo, hi in spec["act_norm"].values():
            assert lo != 0 and lo != -hi
        for name, (lo, hi) in spec["phys_norm"].items():
            assert lo != -hi or abs(hi - np.pi) < 1e-12, name


def kink_share(twin):
    kd = twin.kink_distance()
    return 0.0 if kd is None else float((kd < KINK_MARGIN).double().mean())


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", CASES)
def test_skewed_gpu_inputs_stay_clear_of_kinks(env_name, deadtime, solver, semantics):
    """The inputs of the off-default GPU cases (B = 256, K = 24)"""
    spec = skewed_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, 256, 24, seed=71)
    twin = Twin(env_name, spec, solver, semantics)
    with torch.no_grad():
        twin.sim_ahead(leaves(st), torch.as_tensor(acts), spec["tau"])
    share = kink_share(twin)
    print(f"{env_name} dead={deadtime} {solver} {semantics} skewed: {share:.4f} of the environments within {KINK_MARGIN} of a kink")
    assert share <= KINK_CAP
    if env_name == "pmsm":
        clip = twin.clip_share()
        print(f"pmsm dead={deadtime} {solver} {semantics} skewed: the hexagon clip is active in {clip:.3f} of the action-path evaluations")
        assert 0.01 < clip < 0.5


@pytest.mark.parametrize("env_name,elem,solver,semantics", [c for c in WIDE_CASES if c[1] == 4])
def test_wide_gpu_inputs_stay_clear_of_kinks(env_name, elem, solver, semantics):
    """The inputs of the fp32 wide cases (the fp64 ones exclude nothing)"""
    spec = spec_of(env_name)
    V, sub, st, acts = wide_inputs(env_name, elem, spec)
    twin = Twin(env_name, spec, solver, semantics)
    with torch.no_grad():
        twin.sim_ahead(leaves(st), torch.as_tensor(acts.astype(np.float64)), spec["tau"], sub)
    share = kink_share(twin)
    print(f"{env_name} {solver} {semantics} wide inputs: {share:.4f} of the environments within {KINK_MARGIN} of a kink")
    assert share <= KINK_CAP


def test_the_wide_cases_are_the_44_instantiations():
    assert len(WIDE_CASES) == 44 and len(set(WIDE_CASES)) == 44
    small = [c for c in WIDE_CASES if c[0] in ("pendulum", "mass_spring_damper", "fluid_tank")]
    assert len(small) == 36
    assert sorted(set(c[:3] for c in WIDE_CASES if c not in small)) == [("acrobot", 4, "euler"), ("cartpole", 4, "euler"),
                                                                        ("cartpole", 8, "euler"), ("pmsm", 4, "euler")]


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name,deadtime,sub", [("pendulum", None, 1), ("pendulum", None, 3), ("pmsm", 0, 1), ("pmsm", 1, 1)])
def test_twin_forward_matches_the_oracle_for_one_and_two_actions(env_name, deadtime, sub, solver, semantics):
    spec = case_spec(env_name, deadtime)
    for K in (1, 2):
        st, acts = vjp_inputs(env_name, spec, 64, K, seed=74)
        err, _ = twin_vs_oracle(env_name, spec, solver, semantics, st, acts, spec["tau"], sub)
        print(f"{env_name} dead={deadtime} {solver} {semantics} K={K} substeps={sub}: twin vs oracle {err:.3e}")
        assert err <= 1e-9


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("env_name", ["mass_spring_damper", "cartpole"])
def test_twin_forward_matches_the_oracle_with_three_substeps(env_name, solver, semantics):
    spec = spec_of(env_name)
    st, acts = vjp_inputs(env_name, spec, 64, 5, seed=74)
    err, _ = twin_vs_oracle(env_name, spec, solver, semantics, st, acts, spec["tau"], 3)
    print(f"{env_name} {solver} {semantics} K=5 substeps=3: twin vs oracle {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("pmsm", 0, "rk4"), ("pmsm", 1, "rk4")])
def test_twin_forward_matches_the_oracle_at_half_the_environment_step(env_name, deadtime, solver, semantics):
    """obs_stepsize = action_stepsize = tau / 2: the solver steps by tau / 2 while PMSM's angle prediction and the linspace of
    its "ahead" clips keep the environment's tau"""
    spec = case_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, 64, 24, seed=74)
    err, _ = twin_vs_oracle(env_name, spec, solver, semantics, st, acts, 0.5 * spec["tau"])
    print(f"{env_name} dead={deadtime} {solver} {semantics} step = tau / 2: twin vs oracle {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_dry_tank_inputs_run_dry_and_stay_clear_of_the_margin(solver, semantics):
    """Conditions of the dry-tank GPU cases, from the twin alone: the regime is reached (at least 5 % of the saved rows are exactly
    dry), the gradients are finite, and at most 2 % of the environments ever read a nonzero level within 1e-9 of the range from 0
    (an exactly-zero level is the clamp's own output: both sides take the same branch there). The twin's forward agrees with the
    oracle on these inputs too."""
    spec = spec_of("fluid_tank")
    st, acts = dry_tank_inputs()
    step = DRY_STEP_FACTOR * spec["tau"]
    err, twin = twin_vs_oracle("fluid_tank", spec, solver, semantics, st, acts, step)
    assert err <= 1e-9
    ga, gs, _ = vjp(twin, st, acts, step, 1, g_obs=np.ones((256, 25, 1)), g_last=[np.ones(256)])
    with torch.no_grad():
        _, states, _ = twin.sim_ahead(leaves(st), torch.as_tensor(acts), step)
    dry = (states[0] == 0)
    near = float(twin.near_dry(DRY_MARGIN).double().mean())
    print(f"dry tank {solver} {semantics}: {float(dry.double().mean()):.3f} of the rows dry, {float(dry.any(dim=1).double().mean()):.3f} of the "
          f"environments have a dry row, {near:.4f} read a nonzero level within {DRY_MARGIN} of 0")
    assert float(dry.double().mean()) >= 0.05
    assert near <= KINK_CAP
    assert np.isfinite(ga).all() and np.isfinite(gs[0]).all()
