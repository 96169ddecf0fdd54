"""Input conditions of the randomised closed-loop tests (tests/test_gpu_fuzz_closed_loop.py), without a GPU: a draw must not pass by
being degenerate. Every seed of every family of tests/helpers_fuzz_closed_loop.py runs through the CPU oracle (forward families) or
the float64 twin (reverse family) alone.

1. Clamp share: of the draws with a clip, at least half have between 2 % and 70 % of their action entries changed by the clamp; of the
   policy's ReLU draws at least three quarters have between 10 % and 90 % negative hidden pre-activations.
2. Coverage: every batch size of the list, every model, every solver and every gain form occurs in every family; a draw with >= 4
   control columns; a broadcast-gain reverse draw with A * OW > 2 * EXCENV_MAX_STATIC (several chunks of the batch sum); a policy
   whose widest hidden layer is not the first, and at least a third of the multi-layer networks so.
3. fp32 reverse draws: at most KINK_CAP of the environments within KINK_MARGIN of a kink, in every draw.
The conditions are met by the choice of the seed bases (helpers_fuzz_closed_loop.BASE), never by moving a cap. They are stated for the
default number of draws, whatever EXCENV_FUZZ_SEEDS says: the bases were chosen for that list."""
import functools

import numpy as np
import pytest

import helpers_fuzz_closed_loop as fz
import oracle
from conftest import ENV_NAMES
from helpers_vjp import KINK_CAP

FAMILIES = list(fz.BASE)
N = fz.DEFAULT_SEEDS  # the conditions are those of the default list, for which the seed bases were chosen


@functools.lru_cache(maxsize=None)
def figures(family):
    return [fz.host_figures(family, i) for i in range(N)]


def launched(family):
    """The draws that launch something (the refusal draws of the reverse family do not)"""
    return [f for f in figures(family) if not f["cfg"].get("refusal")]


@pytest.mark.parametrize("family", FAMILIES)
def test_draws_are_reproducible_and_inside_the_limits(family):
    for i in range(N):
        a, sa = fz.draw(family, i)
        b, sb = fz.draw(family, i)
        assert a == b and (sa is None) == (sb is None)
        if sa is not None:
            for group in ("params", "phys_norm", "act_norm"):
                for k in sa[group]:
                    va, vb = (v if isinstance(v, tuple) else (v,) for v in (sa[group][k], sb[group][k]))
                    assert len(va) == len(vb) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(va, vb)), (group, k)
        assert a["B"] in fz.B_LIST and a["B"] <= 1031 and a["K"] in fz.K_LIST and a["K"] <= 7
        assert a["substeps"] in (1, 2, 3) and (fz.model_of(a) != "pmsm" or a["substeps"] == 1)
        assert len(a["control"]) <= fz.MAX_CONTROL and len(set(a["control"])) == len(a["control"])
        if family == "vjp":
            assert not a["batched"] and a["env_name"] != fz.SATURATED and a["cotangents"]
        if family == "policy":
            assert len(a["hidden"]) <= 3 and all(w in fz.WIDTHS for w in a["hidden"])


@pytest.mark.parametrize("family", FAMILIES)
def test_coverage(family):
    cfgs = [f["cfg"] for f in launched(family)]
    models = ENV_NAMES + ([fz.SATURATED] if family != "vjp" else [])
    assert {c["B"] for c in cfgs} == set(fz.B_LIST), sorted({c["B"] for c in cfgs})
    assert {c["env_name"] for c in cfgs} == set(models), sorted({c["env_name"] for c in cfgs})
    assert {c["solver"] for c in cfgs} == set(fz.SOLVERS)
    assert {c["dtype"] for c in cfgs} == set(fz.DTYPES) and {c["K"] for c in cfgs} == set(fz.K_LIST)
    assert max(len(c["control"]) for c in cfgs) >= 4
    if family != "policy":
        assert {c["gain_form"] for c in cfgs} == set(fz.GAIN_FORMS)
        assert {c["integral"] for c in cfgs} == {"none", "zeros", "z0"}
    if family != "vjp":
        assert any(c["batched"] and c["control"] for c in cfgs)  # per-environment properties together with control columns
        assert {c["store_states"] for c in cfgs} == {True, False}
    if family == "vjp":
        wide = [c for c in cfgs if c["gain_form"] == "broadcast" and
                oracle.ENV_DIMS[oracle.ENV_IDS[c["env_name"]]][1] * fz.hf.obs_width(c["env_name"], c["control"]) > 2 * fz.MAX_STATIC]
        assert wide, "no broadcast-gain reverse draw with more than two chunks of the batch sum"
        assert any(c["B"] >= 257 and c["gain_form"] == "broadcast" for c in cfgs)  # several slices of the batch sum
        assert {c["refusal"] for f in figures(family) for c in [f["cfg"]]} >= {"per_env", "saturated"}
        for name in fz.COTANGENTS:
            assert any(name in c["cotangents"] for c in cfgs) and any(name not in c["cotangents"] for c in cfgs), name
    if family == "policy":
        multi = [c for c in cfgs if len(c["hidden"]) >= 1]
        later = [c for c in multi if fz.widest_not_first(c["hidden"])]
        print(f"policy draws: {len(multi)} multi-layer networks, {len(later)} with the widest hidden layer not first")
        assert later and 3 * len(later) >= len(multi)
        assert {len(c["hidden"]) for c in cfgs} == {0, 1, 2, 3} and {c["activation"] for c in cfgs} == {"relu", "tanh"}
        assert any(c["batched"] and max(c["hidden"], default=0) >= 63 for c in cfgs)  # ... with the wide network


@pytest.mark.parametrize("family", FAMILIES)
def test_the_clamp_is_at_work_in_at_least_half_of_the_clipped_draws(family):
    clipped = [f for f in launched(family) if f["cfg"]["clip"] is not None]
    for f in clipped:
        print(f"{family} seed {f['cfg']['seed']}: clip {f['cfg']['clip']}, K {f['cfg']['K']}: clamp share {f['clamped']:.3f}")
    good = [f for f in clipped if 0.02 < f["clamped"] < 0.7]
    assert clipped and 2 * len(good) >= len(clipped), (len(good), len(clipped))


def test_relu_draws_use_both_branches():
    relu = [f for f in launched("policy") if f["cfg"]["activation"] == "relu" and f["cfg"]["hidden"] and f["cfg"]["K"] > 0]
    for f in relu:
        print(f"policy seed {f['cfg']['seed']}: hidden {f['cfg']['hidden']}: negative share {f['negative']:.3f}")
    good = [f for f in relu if 0.1 < f["negative"] < 0.9]
    assert relu and 4 * len(good) >= 3 * len(relu), (len(good), len(relu))


def test_fp32_reverse_draws_stay_under_the_kink_cap():
    fp32 = [f for f in launched("vjp") if f["cfg"]["dtype"] == "float32"]
    assert fp32
    for f in fp32:
        print(f"vjp seed {f['cfg']['seed']}: B {f['cfg']['B']}: excluded {f['excluded']:.4f}")
        assert f["excluded"] <= KINK_CAP, fz.describe(f["cfg"])
