"""EXCENV_OPT_KEEP_CONSTANT_COLUMNS (include/excenv.h, csrc/sim_ahead_body.inc): omega_el is a constant of a PMSM trajectory, so a
launch into buffers that still hold an earlier launch's rows leaves the omega_el state leaf and observation column 2 alone where
row 0 already is what it would store. Checked here: the stores are really gone (a sentinel in rows 1..K survives), everything else
has the bits of a launch into fresh buffers, a wave with one changed environment writes everything, the forms that must ignore the
flag do, and the Python bookkeeping (_placement.TrajSet's stamp) sets the flag exactly when the set's rows are known to be intact.
``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

from exciting_environments_amd import _native
from helpers import NP_DTYPE, make_env, random_state, to_state

pytestmark = pytest.mark.gpu

K = 3
SENTINEL = 12345.0
OBS_COL, LEAF = 2, 6  # Pmsm::observe: ob[2] = normalize(omega_el); omega_el is state leaf 6
KEEP = _native.OPT_KEEP_CONSTANT_COLUMNS
# B = 4096: sixteen workgroups at one environment per lane, four at four. 2^17 with one environment per lane is the batch from which
# rows leave through LDS and the waves of a workgroup store for each other (sim_plan.hpp ROW_SYNC_MIN_BATCH): the vote is the
# workgroup's there. fp64 has two environments per lane at most: a forced 4 runs the V = 2 form.
SHAPES = [(4096, 1), (4096, 2), (4096, 4), (1 << 17, 1)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype is torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Raw:
    """One PMSM call of excenv_sim_ahead_ws on buffers of its own: lane-major trajectories [rows][O][B] / [rows][B]."""

    def __init__(self, B, dtype, vec, states, k=K, seed=11):
        self.env, _props, _keep, spec = make_env("pmsm", B, dtype)
        self.B, self.k, self.vec, self.states, self.dtype = B, k, vec, states, dtype
        self.props, self.keepalive = self.env._props_for(self.env.env_properties, B)
        dev = self.env.device
        self.st_in = [torch.as_tensor(v, dtype=dtype, device=dev) for v in random_state("pmsm", B, NP_DTYPE[dtype], spec, seed)]
        rng = np.random.default_rng(seed + 1)
        self.actions = torch.as_tensor(rng.uniform(-1, 1, (k, 2, B)).astype(NP_DTYPE[dtype]), device=dev)  # lane-major [K][A][B]

    def buffers(self):
        e, B, rows = self.env, self.B, self.k + 1
        new = lambda *s: torch.full(s, float("nan"), dtype=self.dtype, device=e.device)
        return new(rows, 8, B), ([new(rows, B) for _ in range(7)] if self.states else None), [new(B) for _ in range(7)]

    def launch(self, bufs, flags=0, st_in=None, actions=None, a_layout=_native.LAYOUT_LANE_MAJOR):
        e = self.env
        obs, straj, last = bufs
        _native.sim_ahead(e.ENV_ID, e._solver.id, self.dtype, self.B, self.k, 1, self.props, None, float(e.tau), float(e.tau),
                          self.st_in if st_in is None else st_in, self.actions if actions is None else actions, a_layout, obs,
                          straj, _native.LAYOUT_LANE_MAJOR, last, _native.SEM_AHEAD, None,
                          _native.launch_opts(envs_per_lane=self.vec, flags=flags))
        torch.cuda.synchronize()
        return _native.last_launch()

    def put_sentinel(self, bufs):
        obs, straj, _ = bufs
        obs[1:, OBS_COL, :] = SENTINEL
        if self.states:
            straj[LEAF][1:, :] = SENTINEL

    def columns(self, bufs):
        obs, straj, _ = bufs
        return [obs[:, OBS_COL, :]] + ([straj[LEAF]] if self.states else [])

    def others_equal(self, bufs, ref):
        (obs, straj, last), (robs, rstraj, rlast) = bufs, ref
        cols = [c for c in range(8) if c != OBS_COL]
        ok = _same(obs[:, cols, :], robs[:, cols, :]) and _same(obs[0, OBS_COL], robs[0, OBS_COL])
        ok = ok and all(_same(a, b) for a, b in zip(last, rlast))
        if self.states:
            ok = ok and all(_same(straj[j], rstraj[j]) for j in range(7) if j != LEAF) and _same(straj[LEAF][0], rstraj[LEAF][0])
        return ok


def _all_equal(bufs, ref):
    (obs, straj, last), (robs, rstraj, rlast) = bufs, ref
    return (_same(obs, robs) and all(_same(a, b) for a, b in zip(last, rlast))
            and (straj is None or all(_same(a, b) for a, b in zip(straj, rstraj))))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,vec", SHAPES)
@pytest.mark.parametrize("states", [True, False], ids=["states", "obs_only"])
def test_raw_launches_skip_exactly_the_two_columns(dtype, B, vec, states):
    r = _Raw(B, dtype, vec, states)
    fresh = r.buffers()
    form = r.launch(fresh)
    want_v = min(vec, 2) if dtype is torch.float64 else vec
    assert form == f"sim_ahead_kernel (V={want_v})"
    assert not any(torch.isnan(t).any() for t in [fresh[0]] + (fresh[1] or []) + fresh[2])  # every element was written

    # the stores are gone: a sentinel in rows 1..K of the two columns survives a flagged launch; everything else has the fresh bits
    bufs = r.buffers()
    r.launch(bufs)
    assert _all_equal(bufs, fresh)
    r.put_sentinel(bufs)
    assert r.launch(bufs, KEEP) == form  # the flag takes no part in choosing the form
    for col in r.columns(bufs):
        assert bool((col[1:] == SENTINEL).all()), "the constant columns were stored although every row 0 matched"
    assert r.others_equal(bufs, fresh)

    # a launch without the flag overwrites the sentinel everywhere
    r.launch(bufs)
    assert _all_equal(bufs, fresh)

    # one environment with another speed: its wave writes everything — that environment's columns are right in every row — while an
    # environment of another workgroup is still skipped (what lies between is the vote's granularity: not asserted)
    st2 = [t.clone() for t in r.st_in]
    st2[LEAF][300] = st2[LEAF][300] + 50.0
    fresh2 = r.buffers()
    r.launch(fresh2, st_in=st2)
    r.put_sentinel(bufs)
    r.launch(bufs, KEEP, st_in=st2)
    for col, ref in zip(r.columns(bufs), r.columns(fresh2)):
        assert _same(col[:, 300], ref[:, 300])
        assert bool((col[1:, 3000] == SENTINEL).all())
        assert _same(col[0], ref[0])
    assert r.others_equal(bufs, fresh2)


@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float32, 1), (torch.float64, 2)], ids=["f32-4", "f32-1", "f64-2"])
def test_a_nan_speed_equals_itself(dtype, vec):
    """The comparison is one of bit patterns: rows that hold the NaN the launch would store are left alone like any others."""
    r = _Raw(4096, dtype, vec, True)
    st = [t.clone() for t in r.st_in]
    st[LEAF][256:768] = float("nan")
    fresh = r.buffers()
    r.launch(fresh, st_in=st)
    assert bool(torch.isnan(fresh[1][LEAF][:, 256:768]).all()) and bool(torch.isnan(fresh[0][:, OBS_COL, 256:768]).all())
    bufs = r.buffers()
    r.launch(bufs, st_in=st)
    r.put_sentinel(bufs)
    r.launch(bufs, KEEP, st_in=st)
    for col in r.columns(bufs):
        assert bool((col[1:] == SENTINEL).all())
    assert r.others_equal(bufs, fresh)


@pytest.mark.parametrize("dtype,vec", [(torch.float32, 4), (torch.float64, 2)], ids=["f32", "f64"])
def test_row_major_actions_read_by_the_kernel_ignore_the_flag(dtype, vec):
    """The fused form's counted wait needs every store of a row behind a window fill (sim_ahead_body.inc NSTORE): it writes
    everything whatever the flag says. K = 4 here, not 3: that form exists only for action rows of whole 16-byte pieces
    (K * A * 4 bytes in fp32), and it is that form this check is about."""
    r = _Raw(4096, dtype, vec, True, k=4)
    acts_rm = r.actions.permute(2, 0, 1).contiguous()  # [B][K][A]
    fresh = r.buffers()
    assert r.launch(fresh, actions=acts_rm, a_layout=_native.LAYOUT_ENV_MAJOR) == "sim_ahead_kernel (row-major actions fused)"
    lane = r.buffers()
    r.launch(lane)
    assert _all_equal(fresh, lane)  # same bits as the lane-major form
    bufs = r.buffers()
    r.launch(bufs, actions=acts_rm, a_layout=_native.LAYOUT_ENV_MAJOR)
    r.put_sentinel(bufs)
    assert r.launch(bufs, KEEP, actions=acts_rm, a_layout=_native.LAYOUT_ENV_MAJOR) == "sim_ahead_kernel (row-major actions fused)"
    assert _all_equal(bufs, fresh)


# ------------------------------------------------------------------------------------------------------------------ Python level
def _env(dtype=torch.float32, pool=True, B=4096, states=True):
    env, _props, _keep, spec = make_env("pmsm", B, dtype)
    env._SHARED_TRAJ_BYTES = 0  # test sizes through the path of the large outputs
    env._placement.PLACED_BYTES = 0
    env.trajectory_pool = pool
    env.store_state_trajectory = states
    return env, to_state(env, random_state("pmsm", B, NP_DTYPE[dtype], spec, seed=5))


def _actions(env, seed):
    a = env.new_actions_buffer(K)
    g = torch.Generator(device=env.device)
    g.manual_seed(seed)
    a.copy_((torch.rand((K, env.action_dim, env.batch_size), generator=g, device=env.device, dtype=env.dtype) * 2 - 1).permute(2, 0, 1))
    return a


def _leaves(env, st):
    return [getattr(st.physical_state, n) for n in env.STATE_FIELDS]


def _step_both(env, ref_env, state, rstate, a):
    """One chained call of the pooled environment and of the unpooled one; asserts equal bits; returns the new states and the
    pooled call's observation pointer."""
    obs, states, state = env.vmap_sim_ahead(state, a, env.tau, env.tau)
    kept = env.last_constant_columns_kept
    robs, rstates, rstate = ref_env.vmap_sim_ahead(rstate, a, env.tau, env.tau)
    assert ref_env.last_constant_columns_kept is False  # a fresh set per call: nothing to keep
    assert _same(obs, robs)
    if states is not None:
        for x, y in zip(_leaves(env, states), _leaves(ref_env, rstates)):
            assert _same(x, y)
    for x, y in zip(_leaves(env, state), _leaves(ref_env, rstate)):
        assert _same(x, y)
    return state, rstate, kept, obs, states


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("states", [True, False], ids=["states", "obs_only"])
def test_chained_calls_keep_from_the_third_on_and_equal_the_unpooled_run(dtype, states):
    env, state = _env(dtype, states=states)
    ref_env, rstate = _env(dtype, pool=False, states=states)
    kept, ptrs = [], []
    for i in range(6):
        state, rstate, k, obs, st = _step_both(env, ref_env, state, rstate, _actions(env, 100 + i))
        kept.append(k)
        ptrs.append(obs.data_ptr())
        del obs, st
    assert ptrs[0] == ptrs[2] == ptrs[4] and ptrs[1] == ptrs[3] == ptrs[5] and ptrs[0] != ptrs[1]
    assert kept == [False, False, True, True, True, True]  # the first launch into each of the two sets writes everything


def test_an_in_place_write_into_a_returned_array_takes_the_flag_off_once():
    env, state = _env()
    ref_env, rstate = _env(pool=False)
    kept = []
    for i in range(7):
        state, rstate, k, obs, st = _step_both(env, ref_env, state, rstate, _actions(env, 200 + i))
        kept.append(k)
        if i == 2:
            obs.mul_(2)  # set A now holds other values in every column, the constant ones included
        if i == 3:
            st.physical_state.omega_el[:, 1:].zero_()  # set B: through a view of a state leaf
        del obs, st
    assert kept == [False, False, True, True, False, False, True]


def test_a_new_speed_between_calls_is_written():
    env, state = _env()
    ref_env, rstate = _env(pool=False)
    for i in range(6):
        if i in (3, 4):  # the flag is carried (the set is intact) and the kernel finds other values in row 0: it writes them
            w = torch.rand(env.batch_size, device=env.device, dtype=env.dtype) * 500
            if i == 4:
                w = torch.where(torch.arange(env.batch_size, device=env.device) % 1000 == 7, w, state.physical_state.omega_el)
            state.physical_state.omega_el = w
            rstate.physical_state.omega_el = w.clone()
        state, rstate, k, obs, st = _step_both(env, ref_env, state, rstate, _actions(env, 300 + i))
        assert k == (i >= 2)
        del obs, st


def test_the_switch_turns_the_flag_off():
    env, state = _env()
    ref_env, rstate = _env(pool=False)
    env.keep_constant_columns = False
    for i in range(5):
        state, rstate, k, obs, st = _step_both(env, ref_env, state, rstate, _actions(env, 400 + i))
        assert k is False
        del obs, st


def test_calls_under_inference_mode_work_and_never_carry_the_flag():
    """Sets allocated under torch.inference_mode() have no version counters: their launches run as they always did."""
    with torch.inference_mode():
        env, state = _env()
        ref_env, rstate = _env(pool=False)
        for i in range(5):
            state, rstate, k, obs, st = _step_both(env, ref_env, state, rstate, _actions(env, 500 + i))
            assert k is False
            del obs, st
