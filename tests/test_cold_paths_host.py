"""Host half of the cold-path tests (no GPU): tests/helpers_cold.py does what it says.

1. Every special value, after rounding to the number format, lies beyond the threshold its kind is meant to cross; every plain value
   lies inside all of them.
2. The lane pattern holds for 1, 2 and 4 environments per lane: wave 0 mixed, wave 2 clean, wave 3 uniform, the tail special.
3. The CPU oracle and the float64 twin run on the special inputs; outside the huge / NaN / inf environments their outputs are finite.
4. The fp32 reverse comparisons of tests/test_gpu_cold_reverse.py leave out the special environments within KINK_MARGIN of a kink: at
   most KINK_CAP of them (the precedent of tests/test_linearize_host.py; the seed of helpers_cold.REV_SEED is chosen so).
5. The twin's own spread under one ulp of the special angles — what sets the reverse bounds where it exceeds the existing ones — is
   computed here and printed, so that it can be read without a GPU.
6. The same for the closed loop's reverse mode (helpers_cold.feedback_twin_reference: the full affine policy over the special states,
   its clamps counted as kinks): finite gradients, the cap, the spread."""
import numpy as np
import pytest

import oracle
from helpers import ANGLE_STATES
from helpers_cold import (ANGLE_KINDS, NONFINITE_KINDS, REV_K, REV_LANES, all_inside, assignment, build, crosses, kinds_for, reverse_cases,
                          reverse_forms, reverse_id, special_envs, twin_reference, uniform_kind, wave_summary)
from helpers_forms import ACTION_RANGE, B, MODEL_CASES, SEM_ID, linear_spec
from helpers_vjp import KINK_CAP

LINEAR = [m for m, (_, _, lut) in MODEL_CASES.items() if lut is None and m != "pmsm_deadtime0"]


def _bounds(spec, field, batch, e):
    lo, hi = spec["phys_norm"][field]
    return (float(np.broadcast_to(np.asarray(lo, dtype=np.float64), (batch,))[e]),
            float(np.broadcast_to(np.asarray(hi, dtype=np.float64), (batch,))[e]))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("model", LINEAR + ["pmsm_saturated_lds"])
def test_special_values_cross_their_thresholds_and_plain_values_none(model, dtype):
    env_name, _, lut = MODEL_CASES[model]
    if lut is None:
        spec = linear_spec(model)
    else:
        from helpers_guard import saturated_host_spec

        spec = saturated_host_spec(model)[0]
    fields = oracle.STATE_FIELDS[env_name]
    kinds = kinds_for(env_name, dtype, saturated=lut is not None)
    seen = set()
    for uniform in kinds:
        for V in (1, 2, 4):
            b = build(env_name, spec, dtype, B, V, uniform, seed=3, saturated=lut is not None)
            assert b["special"][0].dtype == np.dtype(dtype) and b["mask"].sum() == 5 + 64 * V
            for e in np.flatnonzero(b["mask"]):
                js = np.flatnonzero(b["written"][:, e])
                assert js.size >= 1
                for j in js:
                    lo, hi = _bounds(spec, fields[j], B, e)
                    assert crosses(b["kind"][e], b["special"][j][e], lo, hi, dtype), (b["kind"][e], fields[j], b["special"][j][e])
                    assert (b["kind"][e] in ANGLE_KINDS) == (j in ANGLE_STATES.get(env_name, []))
                seen.add(b["kind"][e])
            # everything that was not written is the plain array, and the plain arrays take every fast path
            for j, f in enumerate(fields):
                same = b["special"][j] == b["plain"][j]
                assert np.array_equal(~same, b["written"][j]) or b["special"][j][~same & ~b["written"][j]].size == 0
                assert np.array_equal(b["special"][j][~b["written"][j]], b["plain"][j][~b["written"][j]])
            assert all_inside(env_name, spec, b["plain"], dtype) is None
    assert seen == set(kinds), (seen, kinds)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_plain_arrays_the_gpu_tests_pass_take_every_fast_path(dtype):
    """Every environment of the arrays the special values are written into: helpers_guard.guard_inputs (forward, every model of the
    sweep, seed 7 as tests/test_gpu_cold_forward.py calls it), helpers_cold.reverse_setup (reverse, every lane width in use) and
    helpers_feedback.main_case (the closed loop)"""
    import helpers_feedback as hf
    from helpers_cold import REV_MODELS, reverse_setup
    from helpers_guard import guard_inputs, guard_spec, saturated_host_spec

    for model in LINEAR + ["pmsm_deadtime0", "pmsm_saturated_lds"]:
        env_name, _, lut = MODEL_CASES[model]
        specs = [guard_spec(model, B), guard_spec(model, B, per_env=True)] if lut is None else [saturated_host_spec(model)[0]]
        for spec in specs:
            plain = guard_inputs(env_name, spec, dtype, B, 3, ())
            assert plain["st"][0].dtype == np.dtype(dtype) and plain["st"][0].shape == (B,)
            assert all_inside(env_name, spec, plain["st"], dtype) is None, model
    for env_name, deadtime in REV_MODELS:
        for V in (1, 16 // np.dtype(dtype).itemsize):
            spec, built, _ = reverse_setup(env_name, deadtime, dtype, V)
            assert built["plain"][0].shape == (V * REV_LANES,)
            assert all_inside(env_name, spec, built["plain"], dtype) is None, (env_name, deadtime, V)
        spec, inp = hf.main_case(env_name, deadtime)
        assert all_inside(env_name, spec, [np.asarray(v).astype(dtype) for v in inp["st"]], dtype) is None, (env_name, deadtime)


@pytest.mark.parametrize("V", [1, 2, 4])
def test_the_lane_pattern_has_mixed_clean_and_uniform_waves(V):
    for batch in (B, V * REV_LANES):
        slots = dict(special_envs(batch, V))
        assert slots["env0"] == [0] and slots["tail"] == [batch - 1]
        assert slots["lane31"][0] // V == 31 and slots["lane31"][0] % V == 0           # the first environment of lane 31
        assert slots["lane63"][0] // V == 63 and slots["lane63"][0] % V == V - 1       # the last environment of lane 63
        assert 64 <= slots["wave1"][0] // V < 128 and slots["wave1"][0] // V not in (64, 127)
        assert sorted({e // V // 64 for e in slots["wave3"]}) == [3] and len(slots["wave3"]) == 64 * V
        a = assignment(batch, V, ["turns", "mod", "zero"], "mod")
        mask = np.zeros(batch, dtype=bool)
        mask[list(a)] = True
        waves = wave_summary(mask, V)
        assert waves[0] == "mixed" and waves[1] == "mixed" and waves[2] == "clean" and waves[3] == "uniform", waves[:4]
        assert waves[-1] == "mixed" and all(w == "clean" for w in waves[4:-1])
        assert {a[e][0] for e in slots["wave3"]} == {"mod"}
        assert len({a[e][0] for s in ("env0", "lane31", "lane63", "wave1", "tail") for e in slots[s]}) == 3


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("model", LINEAR)
def test_the_oracle_runs_on_the_special_inputs(model, dtype):
    """Every solver and semantics, K = 3: no error, and every output of an environment that holds no huge / NaN / inf value is
    finite (so NaN in a kernel's output there is the kernel's)."""
    env_name = MODEL_CASES[model][0]
    spec = linear_spec(model)
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.dtype(dtype).type, B)
    A = len(oracle.ACTION_FIELDS[env_name])
    acts = np.random.default_rng(9).uniform(-ACTION_RANGE, ACTION_RANGE, (B, 3, A)).astype(dtype)
    kinds = kinds_for(env_name, dtype)
    for n, solver in enumerate(("euler", "rk4", "tsit5")):
        b = build(env_name, spec, dtype, B, 1, kinds[n % len(kinds)], seed=3)
        calm = ~np.isin(b["kind"], NONFINITE_KINDS)
        for sem in SEM_ID:
            obs, states, last = oracle.sim_ahead(env_name, solver, b["special"], acts, props, spec["tau"], env_tau=spec["tau"], semantics=SEM_ID[sem])
            assert np.isfinite(obs[calm]).all(), (solver, sem)
            assert all(np.isfinite(s[calm]).all() for s in states) and all(np.isfinite(s[calm]).all() for s in last)
            # and the NaN / inf leaves arrive: those environments' observations are not all finite
            # (but for the tank at -inf: it clamps its level at empty, so every row after the caller's own is an empty tank's)
            for e in np.flatnonzero(np.isin(b["kind"], ("nan", "inf"))):
                if not (env_name == "fluid_tank" and b["special"][0][e] == -np.inf):
                    assert not np.isfinite(obs[e]).all(), (solver, sem, e, b["kind"][e])
        obs, new = oracle.step(env_name, solver, b["special"], acts[:, 0], props, spec["tau"])
        assert np.isfinite(obs[calm]).all()


@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_the_twin_runs_on_the_special_inputs_and_its_spread(case):
    """Per form of the reverse sweep: finite gradients, the excluded share of the fp32 comparison under the cap, and the twin's own
    spread per kind under one ulp of the special angles (printed: it is the bound's second rule)."""
    env_name, deadtime, solver, dtype = case
    kinds = kinds_for(env_name, dtype, reverse=True)
    uniform = uniform_kind(case, kinds)
    for sem, V, sub in reverse_forms(env_name, dtype, solver):
        ref = twin_reference(env_name, deadtime, solver, sem, dtype, V, sub, uniform=uniform)
        flat = np.concatenate([ref["want"][0].ravel()] + [g.ravel() for g in ref["want"][1]])
        assert np.isfinite(flat).all() and np.abs(flat).max() > 0
        assert np.isfinite(ref["obs"]).all()
        assert set(ref["kinds"]) == set(kinds)
        excluded = 1.0 - ref["keep"].mean()
        print(f"cold reverse twin {reverse_id(case)} {sem} V={V} substeps={sub} K={REV_K} uniform={uniform}: excluded {excluded:.4f}, "
              "spread under one ulp " + ", ".join(f"{k} {v:.2e}" for k, v in ref["spread"].items()))
        if dtype == "float32":
            assert excluded <= KINK_CAP, (sem, V, sub, excluded)
    # the one-step inputs: `mod` / `quad64` alone (the trajectory and the step kernel), every kind (the step Jacobians), and the
    # forms of the parameter gradients
    huge = ["mod", "quad64"] if dtype == "float64" else ["mod"]
    n = reverse_cases().index(case)
    variants = [dict(kinds=huge, uniform=huge[n % len(huge)], K=1, last_only=False), dict(kinds=huge, uniform=huge[n % len(huge)], K=1, last_only=True),
                dict(uniform=uniform_kind(case, kinds, shift=1), K=1, last_only=True)]
    for v in variants:
        ref = twin_reference(env_name, deadtime, solver, "step", dtype, 1, 1, **v)
        excluded = 1.0 - ref["keep"].mean()
        print(f"cold reverse twin {reverse_id(case)} step V=1 K=1 {v}: excluded {excluded:.4f}, spread under one ulp "
              + ", ".join(f"{k} {s:.2e}" for k, s in ref["spread"].items()))
        assert np.isfinite(ref["want"][0]).all() and (dtype == "float64" or excluded <= KINK_CAP)
    ref = twin_reference(env_name, deadtime, solver, ("ahead", "step")[n % 2], dtype, 1, 1, uniform=uniform_kind(case, kinds, shift=2))
    assert dtype == "float64" or 1.0 - ref["keep"].mean() <= KINK_CAP


@pytest.mark.parametrize("case", reverse_cases(), ids=reverse_id)
def test_the_closed_loop_twin_runs_on_the_special_inputs_and_its_spread(case):
    """The inputs of tests/test_gpu_cold_reverse.py::test_closed_loop_gradients_with_special_initial_angles through the closed-loop
    twin alone: finite gradients, the clamp at work, the excluded share of the fp32 comparison under the cap (the policy's clamps
    count as kinks), the twin's own spread per kind printed."""
    from helpers_cold import feedback_reverse_subs, feedback_twin_reference

    env_name, deadtime, solver, dtype = case
    kinds = kinds_for(env_name, dtype, reverse=True)
    uniform = uniform_kind(case, kinds, shift=3)
    for sub in feedback_reverse_subs(env_name):
        ref = feedback_twin_reference(env_name, deadtime, solver, dtype, sub, uniform)
        flat = np.concatenate([ref["want"][0].ravel()] + [g.ravel() for g in ref["want"][1]])
        assert np.isfinite(flat).all() and np.abs(flat).max() > 0 and np.isfinite(ref["obs"]).all()
        assert set(ref["kinds"]) == set(kinds)
        assert all_inside(env_name, ref["spec"], ref["built"]["plain"], dtype) is None
        excluded = 1.0 - ref["keep"].mean()
        print(f"cold reverse closed-loop twin {reverse_id(case)} substeps={sub} K={REV_K} uniform={uniform}: excluded {excluded:.4f}, "
              "spread under one ulp " + ", ".join(f"{k} {v:.2e}" for k, v in ref["spread"].items()))
        if dtype == "float32":
            assert excluded <= KINK_CAP, (sub, excluded)
