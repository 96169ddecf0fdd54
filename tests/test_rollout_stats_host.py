"""Host side of the rollout statistics (excenv_row_moments, excenv_episode_stats; `vmap_row_moments`, `vmap_advantage_norm`,
`vmap_episode_stats`, `RunningMoments`; no GPU):
- the header with the two contract blocks and their `_native` mirrors, the exports, ABI 7;
- every refusal by code and whole message, before any launch; B == 0 and N == 0 return OK; the workspace functions against a restatement;
- the kernels exist for both element types without scratch memory;
- the Python methods check shapes and arguments by name;
- the moments twin (helpers_rollout_stats.moments_twin) against a long-double / math.fsum two-pass, the episode twin against a plain
  loop that cuts each lane at its resets, `RunningMoments` over three chunks against the moments of the concatenation;
- the input conditions of the GPU test hold for the shapes it uses."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_rollout_stats as hrs
from exciting_environments_amd import EnvironmentRegistry, _native
from helpers_budget import budget

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64 = ctypes.c_int64
EINVAL, ENULL = -1, -2
MOM, EPI = "excenv_row_moments", "excenv_episode_stats"


def test_header_declares_the_contracts_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "excenv.h")).read()
    assert re.search(r"#define\s+EXCENV_ABI_VERSION\s+7\b", hdr)
    for fn in (MOM, EPI, MOM + "_workspace_bytes", EPI + "_workspace_bytes"):
        assert re.search(rf"\b{fn}\s*\(", hdr), fn
    assert re.search(r"\}\s*excenv_row_moments_t\s*;", hdr) and re.search(r"\}\s*excenv_episode_stats_t\s*;", hdr)
    for line in ("d = (double)x[n][c][b] - shift[c];   S1[c] += d;   S2[c] += d * d",
                 "stats[0] = number of valid samples;  stats[1 + c] = S1[c];  stats[1 + C + c] = S2[c]",
                 "ret = return_in[b] (double; 0 where NULL);   len = steps_in[b] (int32; 0 where NULL)",
                 "if len > 0:  emit (ret, len);  completed[n][b] = ret   else: completed[n][b] = 0",
                 "ret = ret + (double)reward[n];  len += 1;  completed[n][b] = 0",
                 "emit(R, L):  cnt += 1;  SR += R;  SRR += R * R;  SL += L;  mn = R < mn ? R : mn;  mx = R > mx ? R : mx",
                 "first(g) = g * (Tn / G) + min(g, Tn mod G)"):
        assert line in hdr, line
    lib = ctypes.CDLL(_native.library_path())
    for fn in (MOM, EPI, MOM + "_workspace_bytes", EPI + "_workspace_bytes"):
        assert hasattr(lib, fn) and fn in _native.PROTOTYPES, fn
    assert _native.lib().excenv_abi_version() == 7
    assert _native.STRUCTS[_native.RowMoments] == "excenv_row_moments_t" and _native.STRUCTS[_native.EpisodeStats] == "excenv_episode_stats_t"
    assert [n for n, _ in _native.RowMoments._fields_] == ["x", "mask", "shift", "n_columns", "max_groups", "stats", "workspace", "workspace_bytes"]
    assert [n for n, _ in _native.EpisodeStats._fields_] == ["reward", "reset", "return_in", "steps_in", "completed", "return_out", "steps_out",
                                                            "stats", "workspace", "workspace_bytes"]
    assert (_native.MOMENTS_MAX_COLUMNS, _native.EPISODE_STATS) == (hrs.MAX_COLUMNS, hrs.EPISODE_STATS) == (16, 6)
    assert excenvs.RowMoments._fields == ("n", "mean", "var", "sum", "sumsq")
    assert excenvs.EpisodeStats._fields == ("n_episodes", "mean_return", "std_return", "mean_length", "min_return", "max_return",
                                            "episode_return", "episode_steps", "completed")
    assert {"RowMoments", "EpisodeStats", "RunningMoments"} <= set(excenvs.__all__)
    for method in ("vmap_row_moments", "vmap_advantage_norm", "vmap_episode_stats"):
        assert callable(getattr(excenvs.CoreEnvironment, method))


@pytest.mark.parametrize("name", ["row_moments_kernel", "episode_stats_kernel"])
def test_kernels_exist_for_both_types_without_scratch(name):
    res, spans = budget(name)
    for t in "fd":
        hit = [k for k in res if f"{name}I{t}EE" in k]
        assert len(hit) == 1, (t, hit)
        print(hit[0], res[hit[0]], spans.get(hit[0]))
    assert len(res) == 2, sorted(res)
    over = {k: v for k, v in res.items() if v["scratch"] != 0 or v["vgpr"] > 256}
    assert not over, over
    assert all(v["lds"] == 32 for v in res.values()), res  # the four wave values of the tree
    red, _ = budget("rollout_stats_reduce_kernel")
    assert len(red) == 1 and all(v["scratch"] == 0 for v in red.values())


def _mom_record(**kw):
    r = _native.RowMoments(64, 64, 64, 2, 0, 64, 64, 1 << 20)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _epi_record(**kw):
    r = _native.EpisodeStats(64, 64, 64, 64, 64, 64, 64, 64, 64, 1 << 20)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _call(fn, rec, dtype=0, B=4, K=3, no_rec=False):
    lib = _native.lib()
    rc = getattr(lib, fn)(dtype, i64(B), i64(K), None if no_rec else ctypes.byref(rec), None)
    return rc, lib.excenv_last_error().decode()


def test_row_moments_refusals_by_code_and_whole_message():
    """No GPU here: anything that reached a launch would fail differently (EXCENV_EHIP) or crash on the fake pointers."""
    fn = MOM
    assert _call(fn, None, no_rec=True) == (ENULL, f"{fn}: call is NULL")
    for field in ("x", "stats", "workspace"):
        assert _call(fn, _mom_record(**{field: None})) == (ENULL, f"{fn}: call->{field} is NULL")
    for C in (0, 17, -1):
        assert _call(fn, _mom_record(n_columns=C)) == (EINVAL, f"{fn}: call->n_columns must be 1 .. 16 (got {C})")
    assert _call(fn, _mom_record(), dtype=2) == (EINVAL, f"{fn}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(fn, _mom_record(), B=-1) == (EINVAL, f"{fn}: bad B=-1 or N=3")
    assert _call(fn, _mom_record(), K=-2) == (EINVAL, f"{fn}: bad B=4 or N=-2")
    assert _call(fn, _mom_record(max_groups=-1)) == (EINVAL, f"{fn}: call->max_groups must not be negative (got -1; 0: auto)")
    assert _call(fn, _mom_record(), K=1 << 30) == (EINVAL, f"{fn}: N * n_columns = {1 << 30} * 2 rows exceed one launch")
    for B, N, C, mg in ((4, 3, 2, 0), (1028, 9, 5, 0), (1028, 9, 16, 3), (1 << 15, 1000, 1, 0)):
        need = hrs.moments_workspace_bytes(B, N, C, mg)
        msg = f"{fn}: needs an 8-byte aligned workspace of {need} bytes ({fn}_workspace_bytes)"
        assert _call(fn, _mom_record(n_columns=C, max_groups=mg, workspace_bytes=need - 1), B=B, K=N) == (EINVAL, msg)
        assert _call(fn, _mom_record(n_columns=C, max_groups=mg, workspace_bytes=need, workspace=68), B=B, K=N) == (EINVAL, msg)
    assert _call(fn, _mom_record(x=None, n_columns=99), dtype=2) == (ENULL, f"{fn}: call->x is NULL")  # NULL pointers come first
    for rec in (_mom_record(), _mom_record(mask=None, shift=None), _mom_record(n_columns=16)):
        assert _call(fn, rec, B=0)[0] == 0 and _call(fn, rec, K=0)[0] == 0 and _call(fn, rec, B=0, K=0, dtype=1)[0] == 0
    assert _call(fn, _mom_record(stats=None), B=0)[0] == ENULL


def test_episode_stats_refusals_by_code_and_whole_message():
    fn = EPI
    assert _call(fn, None, no_rec=True) == (ENULL, f"{fn}: call is NULL")
    for field in ("reward", "reset", "stats", "workspace"):
        assert _call(fn, _epi_record(**{field: None})) == (ENULL, f"{fn}: call->{field} is NULL")
    assert _call(fn, _epi_record(), dtype=2) == (EINVAL, f"{fn}: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got 2)")
    assert _call(fn, _epi_record(), B=-1) == (EINVAL, f"{fn}: bad B=-1 or K=3")
    assert _call(fn, _epi_record(), K=-2) == (EINVAL, f"{fn}: bad B=4 or K=-2")
    for B in (4, 256, 257, 1 << 15):
        need = hrs.episode_workspace_bytes(B)
        msg = f"{fn}: needs an 8-byte aligned workspace of {need} bytes ({fn}_workspace_bytes)"
        assert _call(fn, _epi_record(workspace_bytes=need - 1), B=B) == (EINVAL, msg)
        assert _call(fn, _epi_record(workspace_bytes=need, workspace=68), B=B) == (EINVAL, msg)
    assert _call(fn, _epi_record(reset=None), dtype=2, B=-1) == (ENULL, f"{fn}: call->reset is NULL")
    for rec in (_epi_record(), _epi_record(return_in=None, steps_in=None, completed=None, return_out=None, steps_out=None)):
        assert _call(fn, rec, B=0)[0] == 0 and _call(fn, rec, K=0)[0] == 0 and _call(fn, rec, B=0, K=0, dtype=1)[0] == 0
    assert _call(fn, _epi_record(stats=None), K=0)[0] == ENULL


def test_workspace_functions_against_the_restatement():
    lib = _native.lib()
    for B in hrs.B_SIZES + (0, 1024, 1025, 1 << 15, (1 << 22) + 1):
        assert lib.excenv_episode_stats_workspace_bytes(B) == hrs.episode_workspace_bytes(B), B
        for N in hrs.N_SIZES + (0, 1000):
            for C in (1, 5, 16):
                for mg in hrs.MAX_GROUPS + (2048, 5000):
                    assert lib.excenv_row_moments_workspace_bytes(B, N, C, mg) == hrs.moments_workspace_bytes(B, N, C, mg), (B, N, C, mg)
    bad = lib.excenv_row_moments_workspace_bytes
    assert bad(-1, 1, 1, 0) == bad(1, -1, 1, 0) == bad(1, 1, 0, 0) == bad(1, 1, 17, 0) == bad(1, 1, 1, -1) == -1
    assert lib.excenv_episode_stats_workspace_bytes(-1) == -1
    assert hrs.groups_of(1028, 9, 0) == (18, 18) and hrs.groups_of(1028, 9, 3) == (18, 3) and hrs.groups_of(1 << 15, 1000, 0) == (32000, 2048)


def test_python_checks_shapes_and_arguments_by_name():
    env = EnvironmentRegistry.PENDULUM.make(batch_size=4, device="cpu")
    B, N = 4, 3
    ok = torch.zeros(B, N)
    for shape in ((3, N), (B,), (B, N, 2, 1)):
        with pytest.raises(ValueError, match=r"vmap_row_moments: x needs to be of shape \(batch_size, n_rows\)"):
            env.vmap_row_moments(torch.zeros(shape))
    for C in (0, 17):
        with pytest.raises(ValueError, match="vmap_row_moments: x needs to have from 1 to 16 columns"):
            env.vmap_row_moments(torch.zeros(B, N, C))
    with pytest.raises(ValueError, match=r"vmap_row_moments: mask needs to be of shape \(batch_size, n_steps\)"):
        env.vmap_row_moments(ok, mask=torch.zeros(B, N + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="vmap_row_moments: shift needs to hold one number per column which is 2"):
        env.vmap_row_moments(torch.zeros(B, N, 2), shift=[0.0, 1.0, 2.0])
    for ddof in (-1, float("nan"), "1", True):
        with pytest.raises(ValueError, match="vmap_row_moments: ddof needs to be a non-negative number"):
            env.vmap_row_moments(ok, ddof=ddof)
    for mg in (-1, 1.5, True):
        with pytest.raises(ValueError, match="vmap_row_moments: max_groups needs to be a non-negative integer"):
            env.vmap_row_moments(ok, max_groups=mg)
    with pytest.raises(ValueError, match=r"vmap_advantage_norm: advantage needs to be of shape \(batch_size, n_steps\)"):
        env.vmap_advantage_norm(torch.zeros(B, N, 1))
    for eps in (0.0, -1e-8, float("inf"), None):
        with pytest.raises(ValueError, match="vmap_advantage_norm: eps needs to be a positive number"):
            env.vmap_advantage_norm(ok, eps=eps)
    flags = torch.zeros(B, N, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"vmap_episode_stats: reward needs to be of shape \(batch_size, n_steps\)"):
        env.vmap_episode_stats(torch.zeros(3, N), flags)
    with pytest.raises(ValueError, match=r"vmap_episode_stats: reset needs to be of shape \(batch_size, n_steps\) which is \(4, 3\)"):
        env.vmap_episode_stats(ok, torch.zeros(B, N + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="vmap_episode_stats: reset is needed"):
        env.vmap_episode_stats(ok, None)
    with pytest.raises(ValueError, match=r"vmap_episode_stats: episode_return needs to be of shape \(batch_size,\)"):
        env.vmap_episode_stats(ok, flags, episode_return=torch.zeros(B + 1))
    with pytest.raises(ValueError, match=r"vmap_episode_stats: episode_steps needs to be of shape \(batch_size,\)"):
        env.vmap_episode_stats(ok, flags, episode_steps=torch.zeros(B, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):  # the arguments are fine: there is no CPU fallback
        env.vmap_row_moments(ok)
    # nothing to launch: the empty statistics
    empty = EnvironmentRegistry.PENDULUM.make(batch_size=0, device="cpu")
    m = empty.vmap_row_moments(torch.zeros(0, N, 2), shift=[1.0, 2.0])
    assert float(m.n) == 0 and m.mean.tolist() == [1.0, 2.0] and m.var.tolist() == [0.0, 0.0]
    e = env.vmap_episode_stats(torch.zeros(B, 0), torch.zeros(B, 0, dtype=torch.bool), episode_steps=torch.arange(B, dtype=torch.int32), per_row=True)
    assert float(e.n_episodes) == 0 and float(e.mean_return) == 0 and float(e.min_return) == math.inf and float(e.max_return) == -math.inf
    assert e.episode_steps.tolist() == [0, 1, 2, 3] and e.episode_return.tolist() == [0.0] * B and tuple(e.completed.shape) == (B, 0)


@pytest.mark.parametrize("dtype", hrs.DTYPES)
def test_moments_twin_against_a_long_double_two_pass(dtype):
    worst = 0.0
    for B, N, C in ((326, 9, 5), (1028, 9, 2), (65, 2, 1), (1, 1, 1)):
        case = hrs.moments_case(B, N, C, dtype)
        for shift in (None, case["shift"]):
            twin = hrs.moments_twin(case["x"], case["mask"], shift)
            valid = ~case["mask"]
            assert twin["n"] == float(valid.sum())
            for c in range(C):
                col = case["x"][:, :, c][valid]
                sh = 0.0 if shift is None else float(shift[c])
                d = col.astype(np.longdouble) - np.longdouble(sh)
                assert np.array_equal(np.sort(d.astype(np.float64)), np.sort(twin["t1"][c]))  # (x - shift is exact or rounded once: the same values)
                for got, terms in ((twin["S1"][c], twin["t1"][c]), (twin["S2"][c], twin["t2"][c])):
                    want, room = hrs.sum_bound(terms)
                    assert abs(got - want) <= room
                    worst = max(worst, abs(got - want) / room if room else 0.0)
                if twin["n"] > 1:
                    # two-pass: the mean in long double, then the centred squares
                    mean = float(np.sum(col.astype(np.longdouble)) / twin["n"])
                    var = float(np.sum((col.astype(np.longdouble) - np.longdouble(mean)) ** 2) / twin["n"])
                    m_ref, m_room, v_ref, v_room = hrs.composed_bounds(twin["n"], twin["t1"][c], twin["t2"][c], sh, 0)
                    assert abs(m_ref - mean) <= m_room + 4 * hrs.U * abs(mean) and abs(v_ref - var) <= v_room + 1e-12 * var
    print(f"moments twin {dtype}: largest |sequential sum - fsum| / bound {worst:.3e}")


@pytest.mark.parametrize("dtype", hrs.DTYPES)
def test_episode_twin_against_a_loop_that_cuts_each_lane_at_its_resets(dtype):
    for B, K in ((326, 9), (65, 2), (1, 1), (63, 9)):
        case = hrs.episode_case(B, K, dtype)
        for carried in (True, False):
            ri, si = (case["return_in"], case["steps_in"]) if carried else (None, None)
            twin = hrs.episode_twin(case["reward"], case["reset"], ri, si)
            done, ret, steps = hrs.episodes_by_cutting(case["reward"], case["reset"], ri, si)
            want = np.zeros((B, K))
            for b, n, total, length in done:
                want[b, n] = total
            assert np.array_equal(want, twin["completed"]) and np.array_equal(ret, twin["ret"]) and np.array_equal(steps, twin["steps"])
            assert twin["stats"][0] == len(done) and twin["stats"][3] == sum(d[3] for d in done)
            assert sorted(twin["R"].tolist()) == sorted(d[2] for d in done) and sorted(twin["L"].tolist()) == sorted(float(d[3]) for d in done)
            if done:
                assert twin["stats"][4] == min(d[2] for d in done) and twin["stats"][5] == max(d[2] for d in done)
            else:
                assert twin["stats"][4] == math.inf and twin["stats"][5] == -math.inf
    # every step a reset: no episode, whatever is carried in without a step
    twin = hrs.episode_twin(np.ones((3, 4)), np.ones((3, 4), bool), np.array([1.0, 2.0, 3.0]), np.zeros(3, np.int32))
    assert twin["stats"][0] == 0 and not twin["completed"].any() and not twin["ret"].any() and not twin["steps"].any()


def _as_moments(x, mask, shift, ddof=0):
    """RowMoments on the CPU from the twin's sums, composed as the method composes them"""
    t = hrs.moments_twin(x, mask, shift)
    n = torch.tensor(t["n"], dtype=torch.float64)
    s1, s2 = torch.as_tensor(t["S1"]), torch.as_tensor(t["S2"])
    sh = torch.zeros_like(s1) if shift is None else torch.as_tensor(np.asarray(shift, np.float64))
    n1 = n.clamp(min=1.0)
    return excenvs.RowMoments(n, sh + s1 / n1, ((s2 - s1 * s1 / n1) / (n - ddof).clamp(min=1.0)).clamp(min=0.0), s1, s2)


def test_running_moments_over_three_chunks_equal_the_moments_of_the_concatenation():
    case = hrs.moments_case(326, 9, 5)
    x, mask = case["x"], case["mask"]
    rm = excenvs.RunningMoments()
    empty = np.ones_like(mask[:, :1])
    for rows, shift in ((slice(0, 2), None), (slice(2, 3), case["shift"]), (slice(3, 9), case["shift"] + 0.5)):
        rm.update(_as_moments(x[:, rows], mask[:, rows], shift))
        rm.update(_as_moments(x[:, :1], empty, None))  # a chunk without a valid sample changes nothing
    valid = ~mask
    assert float(rm.n) == valid.sum()
    for c in range(5):
        col = x[:, :, c][valid].astype(np.longdouble)
        mean = float(col.mean())
        var = float(((col - col.mean()) ** 2).mean())
        assert abs(float(rm.mean[c]) - mean) <= 1e-13 * (1 + abs(mean)) and abs(float(rm.var()[c]) - var) <= 1e-12 * var
        assert abs(float(rm.var(ddof=1)[c]) - var * valid.sum() / (valid.sum() - 1)) <= 1e-12 * var
        assert abs(float(rm.std(eps=1e-8)[c]) - (math.sqrt(var) + 1e-8)) <= 1e-12
    with pytest.raises(ValueError, match="RunningMoments.update: moments of"):
        rm.update(_as_moments(x[:, :, :2], mask, None))


def test_input_conditions_of_the_gpu_tests():
    for dtype in hrs.DTYPES:
        for B in hrs.B_SIZES:
            for N in hrs.N_SIZES:
                for C in hrs.C_SIZES:
                    case = hrs.moments_case(B, N, C, dtype)
                    nf = case["n_fixed"]
                    behind = case["mask"][nf:]
                    if behind.size >= hrs.MIN_SAMPLES:
                        assert 0.1 <= behind.mean() <= 0.3, (B, N, C, behind.mean())
                    if nf:  # the pattern lanes: the first row, the last row, a run, every row
                        m = case["mask"]
                        assert m[0, 0] and m[1, N - 1] and m[2, N // 3:2 * N // 3 + 1].all() and m[3].all()
                    assert np.array_equal(case["x"], case["x"].astype(dtype).astype(np.float64))
                ep = hrs.episode_case(B, N, dtype)
                behind = ep["reset"][ep["n_fixed"]:]
                if behind.size >= hrs.MIN_SAMPLES:
                    assert 0.1 <= behind.mean() <= 0.3
                if B >= 326 and N == 9:
                    assert hrs.episode_conditions(ep) == (True, True, True, True), (B, N, hrs.episode_conditions(ep))
        far = hrs.far_case(326, 9, dtype)
        col = far["x"][:, :, 1][~far["mask"]]
        assert abs(col.mean()) >= 99 * col.std() and 0.1 <= far["mask"][far["n_fixed"]:].mean() <= 0.3
