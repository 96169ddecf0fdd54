"""Generalised advantage estimation on the GPU (excenv_gae: gae_kernel; `vmap_gae`):
1. bit equality with the numpy twin of the contract block (helpers_gae.gae_twin) in fp32 and fp64, over the batch edges, the row
   counts around the prefetch depth, three pairs of discounts, with and without `terminated`, `reset` and `returns`; the first lanes
   are fixed patterns, the others random; the conditions on the inputs are checked on the CPU before the launch;
2. NaN containment: a NaN behind a terminal row or inside a run of resets reaches no output but the returns of the row that holds it;
3. end to end on an episode rollout's views against the float64 direct sum.
Every case prints its figures."""
import numpy as np
import pytest
import torch

import helpers_gae as hgae
import test_gpu_policy_eval as pe
from exciting_environments_amd import _native
from helpers import make_env

pytestmark = pytest.mark.gpu
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = [torch.float32, torch.float64]
_env = pe._env


def lane_major(x, env, dtype=None):
    """[B, n] host array -> [B, n] device view over [n][B] memory (read in place)"""
    x = np.asarray(x)
    t = torch.empty((x.shape[1], x.shape[0]), dtype=dtype or env.dtype, device=env.device).t()
    t.copy_(torch.as_tensor(x))
    return t


def run_gae(env, case, gamma, lam, with_term=True, with_reset=True):
    adv, ret = env.vmap_gae(lane_major(case["reward"], env), lane_major(case["value"], env), gamma, lam,
                            terminated=lane_major(case["terminated"], env, torch.bool) if with_term else None,
                            reset=lane_major(case["reset"], env, torch.bool) if with_reset else None)
    assert _native.last_launch() == "gae_kernel"
    torch.cuda.synchronize()
    B, K = case["reward"].shape
    assert tuple(adv.shape) == (B, K) == tuple(ret.shape) and adv.dtype == env.dtype and adv.grad_fn is None
    assert B == 1 or K == 1 or (tuple(adv.stride()) == (1, B) and tuple(ret.stride()) == (1, B))  # views over [K][B]
    return adv.cpu().numpy(), ret.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("K", hgae.K_SIZES)
@pytest.mark.parametrize("B", hgae.B_SIZES)
def test_equal_bits_with_the_twin(B, K, dtype):
    npdt = NP[dtype]
    case = hgae.gae_case(B, K, np.dtype(npdt).name)
    n = case["n_fixed"]
    # the conditions on the inputs, before any launch
    term, cut = hgae.pattern_flags(K)
    assert np.array_equal(case["reset"][:n], cut[:n]) and np.array_equal(case["terminated"][:n], term[:n])
    if B > n:
        share, free = hgae.input_conditions(case["reset"], n)
        assert 0.1 <= share <= 0.3 and free >= 1, (share, free)
    env = _env(B, dtype)
    runs = 0
    for gamma, lam in hgae.DISCOUNTS:
        for with_term in (True, False):
            for with_reset in (True, False):
                adv, ret = run_gae(env, case, gamma, lam, with_term, with_reset)
                want_a, want_r = hgae.gae_twin(case["reward"], case["value"], gamma, lam, case["terminated"] if with_term else None,
                                               case["reset"] if with_reset else None, npdt)
                assert hgae.same_bits(adv, want_a) and hgae.same_bits(ret, want_r), (gamma, lam, with_term, with_reset)
                runs += 1
        # without `returns`, through the C entry: the same advantages
        rw, vl = lane_major(case["reward"], env), lane_major(case["value"], env)
        tm, rs = lane_major(case["terminated"], env, torch.bool), lane_major(case["reset"], env, torch.bool)
        adv = torch.full((K, B), float("nan"), dtype=dtype, device=env.device)
        hgae.raw_gae(dtype, B, K, rw.data_ptr(), vl.data_ptr(), tm.data_ptr(), rs.data_ptr(), gamma, lam, adv.data_ptr(), None)
        torch.cuda.synchronize()
        want_a, _ = hgae.gae_twin(case["reward"], case["value"], gamma, lam, case["terminated"], case["reset"], npdt)
        assert hgae.same_bits(adv.t().cpu().numpy(), want_a)
        runs += 1
    print(f"gae B={B} K={K} {np.dtype(npdt).name}: {runs} launches with the twin's bits (seed {case['seed']}, {n} pattern lanes)")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("K", [9, 40])
def test_nan_behind_terminal_rows_and_inside_reset_runs_is_contained(K, dtype):
    """Flags as an episode rollout writes them (terminated[n] sets reset[n + 1]). NaN in value[n + 1] behind every terminated[n], and
    in reward[n] and value[n + 1] at every reset[n] whose next row is also a reset. The block reads such a value[n + 1] once: as
    returns[n + 1] of the reset row n + 1. Nothing else may hold a NaN."""
    B, npdt = 326, NP[dtype]
    base = hgae.gae_case(B, K, np.dtype(npdt).name)
    term, cut = base["terminated"].copy(), base["reset"].copy()
    cut[:, 1:] |= term[:, :-1]
    reward, value = base["reward"].copy(), base["value"].copy()
    value[:, 1:][term] = np.nan
    runs = cut[:, :-1] & cut[:, 1:]
    reward[:, :-1][runs] = np.nan
    value[:, 1:K][runs] = np.nan
    expect = np.isnan(value[:, :K]) & cut
    assert np.array_equal(expect, np.isnan(value[:, :K])) and expect.sum() > 0 and runs.sum() > 0 and term[:, K - 1].any()
    case = dict(reward=reward, value=value, terminated=term, reset=cut)
    env = _env(B, dtype)
    for gamma, lam in hgae.DISCOUNTS:
        adv, ret = run_gae(env, case, gamma, lam)
        want_a, want_r = hgae.gae_twin(reward, value, gamma, lam, term, cut, npdt)
        assert np.isfinite(adv).all() and np.array_equal(np.isnan(ret), expect)
        assert hgae.same_bits(adv, want_a) and hgae.same_bits(ret, want_r)
    print(f"gae NaN containment K={K} {np.dtype(npdt).name}: {int(np.isnan(value).sum())} NaN values, {int(np.isnan(reward).sum())} NaN "
          f"rewards in, {int(expect.sum())} NaN returns out (the reset rows that hold them), no NaN advantage")


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_on_an_episode_rollouts_views_against_the_direct_sum(dtype):
    """fp64: within 1e-12 of the largest advantage. fp32: the kernel's contract is the twin's bits, and the twin is one evaluation of
    the block with one rounding per operation; every such evaluation lies within helpers_gae.forward_bound of the exact recurrence
    (derived there: the roundings of the two multiply-adds and the subtraction of every row, and of the two discounts, carried by
    gamma lambda per row). The bound asserted is that forward bound, stated as a multiple of the twin's own distance to the direct
    sum; the multiple is measured here on the CPU from the twin and printed, and nothing of it comes from the kernel."""
    npdt = NP[dtype]
    env, policy, inp, noise, ro = pe._episodes(dtype)
    B, K = ro.reward.shape
    gamma, lam = 0.99, 0.95
    value = np.random.default_rng(19).normal(size=(B, K + 1)).astype(npdt).astype(np.float64)
    adv, ret = env.vmap_gae(ro.reward, lane_major(value, env), gamma, lam, terminated=ro.terminated, reset=ro.reset)
    assert _native.last_launch() == "gae_kernel"
    torch.cuda.synchronize()
    rew, term, cut = ro.reward.cpu().numpy().astype(np.float64), ro.terminated.cpu().numpy(), ro.reset.cpu().numpy()
    want_a, want_r = hgae.gae_direct(rew, value, gamma, lam, term, cut)
    top = float(np.abs(want_a).max())
    got_a, got_r = adv.cpu().numpy(), ret.cpu().numpy()
    twin_a, twin_r = hgae.gae_twin(rew, value, gamma, lam, term, cut, npdt)
    d_twin = float(np.abs(twin_a.astype(np.float64) - want_a).max()) / top
    d = float(np.abs(got_a.astype(np.float64) - want_a).max()) / top
    dr = float(np.abs(got_r.astype(np.float64) - want_r).max()) / top
    label = f"gae on episodes E2 {np.dtype(npdt).name}: reset share {cut.mean():.3f}, terminated share {term.mean():.3f}, largest advantage {top:.3e}"
    assert 0.0 < cut.mean() < 1.0 and top > 0
    if dtype == torch.float64:
        print(f"{label}; advantages within {d:.3e}, returns within {dr:.3e} of the direct sum (bound 1e-12); the twin {d_twin:.3e}")
        assert d <= 1e-12 and dr <= 1e-12
    else:
        bound = hgae.forward_bound(rew, value, gamma, lam, term, cut, npdt)
        assert np.all(np.abs(twin_a.astype(np.float64) - want_a) <= bound) and d_twin > 0
        multiple = float(bound.max()) / top / d_twin
        print(f"{label}; the twin within {d_twin:.3e} of the direct sum, the forward bound {float(bound.max()) / top:.3e} = {multiple:.2f} "
              f"times that; advantages within {d:.3e}, returns within {dr:.3e}")
        assert d <= multiple * d_twin and np.all(np.abs(got_a.astype(np.float64) - want_a) <= bound)
        assert dr <= multiple * d_twin + 2.0 ** -24 * float(np.abs(want_r).max()) / top  # the one further rounding of carry + value
    assert hgae.same_bits(got_a, twin_a) and hgae.same_bits(got_r, twin_r)
