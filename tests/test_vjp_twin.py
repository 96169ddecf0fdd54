"""The float64 torch twin (tests/helpers_vjp.py) is validated before anything is compared with it: its forward observations
against the fp64 CPU oracle, both semantics, every model and solver, PMSM with dead time 0 and 1 — 64 environments x K = 50,
1e-9 on normalised observations (both sides are fp64 and differ by summation order only; 1e7 x eps leaves room for 50 steps and
the acrobot's amplification). The same file asserts, on the twin's own forward of the GPU tests' inputs, that at most 2 % of the
environments come within the kink margin: the inputs are known to be usable before a GPU is involved."""
import numpy as np
import pytest
import torch

import oracle
from conftest import ENV_NAMES
from helpers import spec_of
from helpers_vjp import KINK_CAP, KINK_MARGIN, SEM, Twin, leaves, vjp_inputs

CASES = [(e, None) for e in ENV_NAMES if e != "pmsm"] + [("pmsm", 0), ("pmsm", 1)]
SOLVERS = ["euler", "rk4", "tsit5"]


def case_spec(env_name, deadtime):
    spec = spec_of(env_name)
    if deadtime is not None:
        spec["params"]["deadtime"] = deadtime
    return spec


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
