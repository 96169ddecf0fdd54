"""The path tracer of tests/helpers_rng.py against the oracle, and the conditions the batches of tests/test_gpu_rng_paths.py have to
meet — all of them statements about the oracle's outputs (oracle/oracle_rng.inc), checked here on the CPU and never fitted to a
device result. Run with ``-s`` to see the path counts and the fragile share."""
import numpy as np
import pytest

import oracle
import helpers_rng as hr
from test_oracle_rng import _randint_bigint

DTYPES = [np.float32, np.float64]
REBUILD_RTOL = {np.float32: 1e-6, np.float64: 1e-12}
FRAGILE_SHARE_CAP = 2e-4  # of the pool; a condition on the reference: recorded, not tuned


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_tracer_follows_the_oracles_path(dtype):
    """Every key of the pool the rare batch is drawn from: the gamma samples rebuilt from the traced V and the boost are the
    oracle's, and so is the disc point — a tracer that left a loop one round early or late would hold another sample."""
    seed = hr.rare_batch(dtype)["seed"]
    keys, tr = hr.pool(dtype, seed)
    assert keys.shape == (hr.POOL, 2) and (tr["rounds"] >= 1).all() and np.isfinite(tr["margin"]).all()
    want = oracle.gamma(tr["gamma_key"], 0.5, 2, dtype)
    assert (want > 0).all()
    worst_gamma, worst_disc = _rel(tr["gamma"], want), _rel(tr["disc"], oracle.ball2(tr["ball_key"], dtype))
    print(f"\n{np.dtype(dtype).name}: rebuilt gamma within {worst_gamma:.2e}, disc within {worst_disc:.2e} (relative) of the oracle's")
    assert worst_gamma <= REBUILD_RTOL[dtype] and worst_disc <= REBUILD_RTOL[dtype]
    # the tree above the ball: the oracle's PMSM state on the default box is the disc point times 250 A, mirrored at i_d = 0
    from helpers import spec_of

    spec = spec_of("pmsm")
    n = 4096
    props, keep = oracle.make_props("pmsm", spec["params"], spec["phys_norm"], spec["act_norm"], dtype, n)
    st, _ = oracle.random_state("pmsm", keys[:n], props, dtype)
    mt = hr.pmsm_mirror_terms(keys[:n], spec, dtype)
    assert np.array_equal(st[3], mt["i_d"]) and np.array_equal(st[4], mt["i_q"])
    assert _rel(np.abs(tr["disc"][:n, 1]) * 250.0, np.abs(st[4])) <= REBUILD_RTOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_rare_batch_holds_the_rare_paths_and_no_fragile_key(dtype):
    rb = hr.rare_batch(dtype)
    B, pool = rb["B"], rb["pool"]
    cls, rare = rb["cls"], rb["rare"]
    n_redo, n_rounds = int((cls == "redo").sum()), int((rb["rounds"].max(axis=1) >= 3).sum())
    print(f"\n{np.dtype(dtype).name}: seed {rb['seed']}; pool of {hr.POOL}: {pool['redo']} redo keys, {pool['rounds2']} of two or more "
          f"rounds, {pool['rounds3']} of three or more, {pool['rounds4']} of four or more, {pool['fragile']} fragile "
          f"(share {pool['fragile_share']:.2e}); batch of {B}: {n_redo} redo, {n_rounds} of three or more rounds, "
          f"deepest {int(rb['rounds'].max())} rounds, most redraws {int(rb['redo'].max())}, smallest margin {rb['margin'].min():.2e}")
    assert B <= 1031 and rb["keys"].shape == (B, 2)
    assert n_redo >= hr.MIN_REDO and n_rounds >= hr.MIN_ROUNDS3 and rb["rounds"].max() >= 4
    assert pool["fragile_share"] <= FRAGILE_SHARE_CAP
    assert (rb["margin"] >= hr.fragile_below(dtype)).all()  # zero fragile keys in the batch
    assert np.array_equal(rare, cls != "plain")
    # traced afresh from the batch's own keys: the stored facts belong to these keys; the replacement batch is ordinary throughout
    again = hr.trace_ball(rb["keys"], dtype)
    assert np.array_equal(again["rounds"], rb["rounds"]) and np.array_equal(again["redo"], rb["redo"]) and not again["fragile"].any()
    plain = hr.trace_ball(rb["plain_keys"], dtype)
    assert (hr.classify(plain) == "plain").all() and not plain["fragile"].any()
    assert np.array_equal(rb["plain_keys"][~rare], rb["keys"][~rare])
    assert len({tuple(k) for k in rb["keys"]}) == B
    # the lane pattern: environment 0 and B - 1 rare and alone in their waves, wave 1 one rare key, wave 2 clean, wave 3 redo only
    kinds = hr.wave_kinds(rare)
    assert rare[0] and rare[B - 1] and rare[:64].sum() == 1 and rare[64:128].sum() == 1 and rare[B - B % 64:].sum() == 1 and B % 64
    assert kinds[2] == "clean" and kinds[3] == "uniform" and (cls[192:256] == "redo").all()
    assert all(k == "mixed" for i, k in enumerate(kinds) if i not in (2, 3))
    assert rb["rounds"][0].max() >= 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_skewed_per_environment_box_fires_every_mirror_term(dtype):
    B = 257
    keys, tr, seed = hr.plain_keys(dtype, B)
    spec, plan = hr.per_env_spec("pmsm", B)
    assert {n for n, _ in plan} == {"i_d", "i_q"} and len(plan) == 3
    props, keep = oracle.make_props("pmsm", spec["params"], spec["phys_norm"], spec["act_norm"], dtype, B)
    st, _ = oracle.random_state("pmsm", keys, props, dtype)
    mt = hr.pmsm_mirror_terms(keys, spec, dtype)
    assert np.array_equal(st[3], mt["i_d"]) and np.array_equal(st[4], mt["i_q"])  # the terms below are the oracle's
    share = mt["fired"].mean(axis=1)
    print(f"\n{np.dtype(dtype).name}: seed {seed}, {int(tr['fragile'].sum())} fragile keys of {B}; mirror terms fire in "
          f"{', '.join(f'{s:.1%}' for s in share)} of the environments (i_d high, i_d low, i_q high, i_q low); i_max is "
          f"{np.bincount(mt['bounds'].argmax(axis=0), minlength=4).tolist()} times |i_d min|, |i_d max|, |i_q min|, |i_q max|")
    assert (share >= 0.05).all()
    assert int(tr["fragile"].sum()) <= 1
    # i_max is one bound's magnitude and no other's: reading the wrong leaf, or environment 0's, gives another number
    srt = np.sort(mt["bounds"], axis=0)
    assert (srt[-1] > srt[-2]).all() and len(np.unique(mt["bounds"].argmax(axis=0))) >= 3
    assert (np.abs(mt["i_max"][1:] - mt["i_max"][0]) > 1e-3).all()


@pytest.mark.parametrize("env_name", list(oracle.ENV_IDS))
def test_per_environment_boxes_differ_between_environments(env_name):
    B = 257
    spec, plan = hr.per_env_spec(env_name, B)
    assert len(plan) == (2 if env_name == "fluid_tank" else 3)
    for name, side in plan:
        v = spec["phys_norm"][name][side]
        assert isinstance(v, np.ndarray) and v.shape == (B,) and len(np.unique(v)) == B
    for name, (lo, hi) in spec["phys_norm"].items():
        assert (np.asarray(hi) > np.asarray(lo)).all(), name


def test_hold_ranges_against_the_big_integer_restatement():
    keys = oracle.split(oracle.prng_key(2025), 48)
    for lo, hi in hr.HOLD_RANGES + hr.WIDE_HOLD_RANGES:
        want32 = [_randint_bigint(k, 2, lo, hi, 32) for k in keys]
        want64 = [_randint_bigint(k, 2, lo, hi, 64) for k in keys]
        got32, got64 = oracle.randint(keys, 2, lo, hi), oracle.randint64(keys, 2, lo, hi)
        if hi - lo <= hr.INT32_MAX:
            assert got32.tolist() == want32, (lo, hi)
        else:  # the int32 form's sum wraps into int32 like the span does
            wrap = lambda v: (v + (1 << 31)) % (1 << 32) - (1 << 31)
            assert got32.tolist() == [[wrap(v) for v in row] for row in want32], (lo, hi)
        assert got64.tolist() == want64, (lo, hi)
        for got in (got32, got64):
            if hi > lo:
                assert got.min() >= lo and got.max() < hi, (lo, hi)
            assert len(np.unique(got)) == 1 if hr.span_of(lo, hi) == 1 else len(np.unique(got)) >= 2, (lo, hi)
            if hr.span_of(lo, hi) == 1:
                assert (got == lo).all()
