"""The twin's parameter gradients (tests/helpers_vjp_params.py) on the CPU, before the GPU kernel is compared with them: autograd
against the twin's own central difference, the share of environments near a kink, and that every differentiable leaf is visible
in the inputs the GPU tests use. B = 256, K = 24, skewed specs, every case x solver x semantics."""
import numpy as np
import pytest

from helpers_vjp import CASES, DRY_MARGIN, DRY_STEP_FACTOR, KINK_CAP, SOLVERS, cotangents, dry_tank_inputs
from helpers_vjp_params import ParamTwin, direction, quotient_err, reference, twin_directional

ALL = [(e, d, s, sem) for e, d in CASES for s in SOLVERS for sem in ("ahead", "step")]


@pytest.mark.parametrize("env_name,deadtime,solver,semantics", ALL)
def test_autograd_matches_the_twins_own_central_difference(env_name, deadtime, solver, semantics):
    """Per environment, direction = all differentiable parameters at once (each scaled by its own value times a fixed factor in
    +-[0.5, 1.5]), relative step 1e-5, error relative to the batch's largest quotient. Measured when the helper was written:
    7.8e-11 ... 1.2e-8 (worst: pendulum); bound 1e-7 = 10 x that, and 10 x below the GPU finite-difference bound."""
    dd, fd, keep = twin_directional(env_name, deadtime, solver, semantics)
    err = quotient_err(dd, fd, keep)
    print(f"{env_name} dead={deadtime} {solver} {semantics}: twin autograd vs central difference {err:.3e}")
    assert err <= 1e-7


@pytest.mark.parametrize("env_name,deadtime,solver,semantics", ALL)
def test_excluded_share_and_visibility_of_every_leaf(env_name, deadtime, solver, semantics):
    ref = reference(env_name, deadtime, solver, semantics)
    excluded = 1.0 - ref["keep"].mean()
    assert excluded <= KINK_CAP, excluded
    spec, want = ref["spec"], ref["want"][0]
    vis = {k: float(np.max(np.abs(want[k] * float(spec["params"][k])))) for k in ref["names"]}
    print(f"{env_name} dead={deadtime} {solver} {semantics}: excluded {excluded:.4f}, max |gradient x value| "
          + ", ".join(f"{k} {v:.2e}" for k, v in vis.items()))
    assert set(direction(ref["names"])) == set(ref["names"])
    for k, v in vis.items():
        if env_name == "acrobot" and k == "l_2":
            assert v == 0.0 and not want[k].any()  # f never reads l_2
        else:
            assert v > 0.0, k
    if env_name == "pmsm":  # u_dc is visible only where the hexagon clip is active
        assert 0.01 < ref["clip_share"] < 0.5, ref["clip_share"]


@pytest.mark.parametrize("semantics", ["ahead", "step"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_dry_tank_inputs_have_no_level_within_the_margin(solver, semantics):
    """The GPU dry-tank comparison excludes nothing: no environment reads a nonzero level within DRY_MARGIN of 0"""
    from helpers import spec_of

    spec = spec_of("fluid_tank")
    st, acts = dry_tank_inputs()
    tw = ParamTwin("fluid_tank", spec, solver, semantics, st, acts, DRY_STEP_FACTOR * spec["tau"])
    assert not tw.twin.near_dry(DRY_MARGIN).any()
    want = tw.grads(cotangents(np.random.default_rng(5), acts.shape[0], acts.shape[1] + 1, 1, 1))
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in want.values())
