"""Host side of EXCENV_OPT_KEEP_CONSTANT_COLUMNS (include/excenv.h): the flag exists in the header and in the binding without a new
ABI version, it takes no part in routing, and the bookkeeping that decides when a launch may carry it (_placement.TrajSet's stamp,
TrajectoryPlacement.launch_into) says yes only for a pooled set whose buffers nothing has written since this environment's last
lane-major launch into it. No kernel is launched here: the buffers are stand-ins that have a version counter and nothing else."""
import re
from types import SimpleNamespace

import pytest
import torch

from exciting_environments_amd import EnvironmentRegistry, _native
from exciting_environments_amd._placement import TrajectoryPlacement, TrajSet
from test_native_binding import HEADER, ROUTES, _LAYOUT_ID, _LAYOUT_NAME


def test_the_flag_is_mirrored_and_the_abi_version_stays():
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+EXCENV_([A-Z_0-9]+)\s+\(?(-?\d+)\)?", hdr)}
    assert values["OPT_KEEP_CONSTANT_COLUMNS"] == 2 == _native.OPT_KEEP_CONSTANT_COLUMNS
    assert values["OPT_NO_FUSED_ACTIONS"] == 1 == _native.OPT_NO_FUSED_ACTIONS  # distinct bits
    assert values["ABI_VERSION"] == 7 == _native.ABI_VERSION == _native.lib().excenv_abi_version()


def test_the_library_accepts_the_flag_and_still_refuses_unknown_bits():
    """Argument checks only (B == 0 returns before anything is launched; no device is touched)."""
    lib = _native.lib()
    env = EnvironmentRegistry.PMSM.make(batch_size=4, device="cpu")
    props, _keep = env._props_for(env.env_properties, 4)
    import ctypes

    S = env.physical_state_dim
    ptrs = (ctypes.c_void_p * S)(*([16] * S))  # non-NULL, never dereferenced

    def call(flags):
        o = _native.launch_opts(0, 0, 0, flags)
        return lib.excenv_sim_ahead_ws(env.ENV_ID, 0, 0, 0, 3, 1, ctypes.byref(props), None, 1e-4,
                                       1e-4, ptrs, 16, _native.LAYOUT_LANE_MAJOR, 16, ptrs, _native.LAYOUT_LANE_MAJOR, ptrs,
                                       _native.SEM_AHEAD, None, None, 0, ctypes.byref(o), None)

    assert call(0) == 0
    assert call(_native.OPT_KEEP_CONSTANT_COLUMNS) == 0
    assert call(_native.OPT_KEEP_CONSTANT_COLUMNS | _native.OPT_NO_FUSED_ACTIONS) == 0
    assert call(4) != 0 and b"unknown bits" in lib.excenv_last_error()


@pytest.mark.parametrize("spec, want", ROUTES, ids=[" ".join(map(str, s)).replace(" ", "-") for s, _ in ROUTES])
def test_routing_does_not_know_the_switch(spec, want):
    """_route decides what tests/test_native_binding.py pins, whatever env.keep_constant_columns says: the flag is added at launch
    time, to the launch into a pooled set alone."""
    B, K, sub, traj, act, gym, out, fused, ws, opts, states, sem = spec
    got = []
    for switch in (True, False):
        env = EnvironmentRegistry.PENDULUM.make(batch_size=B, device="cpu")
        assert env.keep_constant_columns is True and env.last_constant_columns_kept is False  # the defaults
        env.keep_constant_columns = switch
        env.traj_layout, env.env_major_fused, env.env_major_workspace = _LAYOUT_NAME[traj], bool(fused), bool(ws)
        env.store_state_trajectory, env.sim_ahead_semantics = bool(states), sem
        env.launch_opts = None if opts is None else _native.launch_opts(*opts)
        props, _keep = env._props_for(env.env_properties, B)
        a = [torch.zeros(16) for _ in range(3)]
        try:
            t_layout, want_states, o, ws_bytes, provider = env._route(B, K, sub, _LAYOUT_ID[act], bool(gym), bool(out), True, props,
                                                                      a[0], a[1:])
        except (ValueError, AssertionError) as e:
            got.append((type(e).__name__, None, None))
            continue
        assert t_layout == _LAYOUT_ID[traj] and want_states == bool(states)
        got.append((provider, None if o is None else (o.envs_per_lane, o.env_major_mode, o.lds_pad_bytes, o.flags), ws_bytes > 0))
    assert got == [want, want]


class _Buf:
    """What the stamp reads of a tensor: the version counter every in-place torch operation through any view moves."""

    def __init__(self):
        self._version = 0


def _fake_set(states=True):
    ts = TrajSet(key=("fake",))
    ts.obs_buf, ts.st_buf = _Buf(), (_Buf() if states else None)
    ts.obs_ptr, ts.traj_ptrs, ts.last_ptrs = 1, 2, 3
    return ts


def _placement():
    env = SimpleNamespace(trajectory_placement="auto", trajectory_pool=True, dtype=torch.float32, device=torch.device("cpu"))
    return TrajectoryPlacement(env)


def _launcher(log):
    def launch(o_ptr, t_ptrs, l_ptrs, keep=False):  # the shape of _trajectory.py's closure
        log.append(((o_ptr, t_ptrs, l_ptrs), keep))
    return launch


@pytest.mark.parametrize("states", [True, False])
def test_stamp_first_launch_steady_state_and_version_bumps(states):
    pl, ts, log = _placement(), _fake_set(states), []
    launch = _launcher(log)
    go = lambda **kw: pl.launch_into(ts, launch, 1000, kw.get("lane_major", True), kw.get("allow", True), kw.get("capturing", False))
    assert not ts.constant_columns_intact()
    assert go() is False                      # the first launch into a new set: nobody has written its columns yet
    assert ts.constant_columns_intact()
    assert go() is True and go() is True      # steady state
    assert [k for _, k in log] == [False, True, True] and all(p == (1, 2, 3) for p, _ in log)
    ts.obs_buf._version += 1                  # obs.mul_(2) through any view of the observation buffer
    assert not ts.constant_columns_intact()
    assert go() is False and go() is True     # ... the next launch writes everything and stamps again
    if states:
        ts.st_buf._version += 1               # an in-place write into a state leaf
        assert go() is False and go() is True
    assert go(allow=False) is False           # env.keep_constant_columns = False: no flag, and no stamp is kept at all
    assert ts.const_stamp is None
    assert go() is False and go() is True     # switched on again: one full launch, then steady state


def test_a_launch_that_cannot_promise_anything_leaves_no_stamp():
    pl, ts, log = _placement(), _fake_set(), []
    launch = _launcher(log)
    assert pl.launch_into(ts, launch, 1000, True, True, False) is False
    # a graph capture: the launch runs when the graph is replayed — never flagged, and nothing is known afterwards
    assert pl.launch_into(ts, launch, 1000, True, True, True) is False
    assert ts.const_stamp is None
    assert pl.launch_into(ts, launch, 1000, True, True, False) is False and ts.constant_columns_intact()
    # row-major trajectories: never flagged, never stamped
    assert pl.launch_into(ts, launch, 1000, False, True, False) is False and ts.const_stamp is None
    # a launch that raises leaves no promise behind

    def boom(*a):
        raise RuntimeError("launch failed")

    assert pl.launch_into(ts, launch, 1000, True, True, False) is False and ts.constant_columns_intact()
    with pytest.raises(RuntimeError):
        pl.launch_into(ts, boom, 1000, True, True, False)
    assert ts.const_stamp is None


def test_a_new_set_and_probe_launches_never_carry_the_flag():
    pl, log = _placement(), []
    launch = _launcher(log)
    old = _fake_set()
    pl.launch_into(old, launch, 1000, True, True, False)
    assert pl.launch_into(old, launch, 1000, True, True, False) is True
    # a replacement set of the same key starts without a stamp, whatever its predecessor had
    new = _fake_set()
    assert new.const_stamp is None and not new.constant_columns_intact()
    # placement probes call the closure with the three pointers alone (acquire: time_launch) — into candidate blocks, unflagged —
    # and leave no stamp: only launch_into stamps
    del log[:]
    launch(new.obs_ptr, 77, new.last_ptrs)
    assert log == [((1, 77, 3), False)] and new.const_stamp is None
    assert pl.launch_into(new, launch, 1000, True, True, False) is False
    assert pl.launch_into(new, launch, 1000, True, True, False) is True
    assert old.constant_columns_intact()  # the other set's stamp is its own


def test_real_tensors_move_the_counter_through_every_view():
    """The property the stamp rests on, with torch's own tensors (CPU): views share their base's version counter."""
    ts = TrajSet(key=("cpu",))
    ts.obs_buf, ts.st_buf = torch.zeros(4, 8, 16), torch.zeros(7, 4, 16)
    obs_view = ts.obs_buf.permute(2, 0, 1)
    leaf = ts.st_buf.as_strided((7, 16, 4), (64, 1, 16)).unbind(0)[6]
    ts.stamp_constant_columns()
    assert ts.constant_columns_intact()
    _ = obs_view * 2 + leaf.sum()  # reading changes nothing
    assert ts.constant_columns_intact()
    obs_view.mul_(2)
    assert not ts.constant_columns_intact()
    ts.stamp_constant_columns()
    leaf[3, 1] = 5.0
    assert not ts.constant_columns_intact()
    ts.stamp_constant_columns()
    obs_view.detach()[0].zero_()
    assert not ts.constant_columns_intact()


def test_buffers_made_under_inference_mode_are_never_stamped():
    """Inference tensors have no version counter (reading it raises): their history cannot be known, so launches into such a set work
    as before this flag existed — no stamp, no flag, no exception — whatever the switch says."""
    with torch.inference_mode():
        ts = TrajSet(key=("inference",))
        ts.obs_buf, ts.st_buf = torch.zeros(4, 8, 16), torch.zeros(7, 4, 16)
        ts.obs_ptr, ts.traj_ptrs, ts.last_ptrs = 1, 2, 3
        assert ts.obs_buf.is_inference()
        with pytest.raises(RuntimeError):
            ts.obs_buf._version
        pl, log = _placement(), []
        for allow in (True, True, False, True):
            assert pl.launch_into(ts, _launcher(log), 1000, True, allow, False) is False
            assert ts.const_stamp is None and not ts.constant_columns_intact()
        ts.obs_buf.mul_(2)  # handed out and written in that mode: still nothing known
        assert pl.launch_into(ts, _launcher(log), 1000, True, True, False) is False
    assert pl.launch_into(ts, _launcher(log), 1000, True, True, False) is False  # the same set used outside the mode again
    assert [k for _, k in log] == [False] * 6
    # one inference buffer is enough (observations made outside, state block inside)
    mixed = TrajSet(key=("mixed",))
    mixed.obs_buf = torch.zeros(4, 8, 16)
    with torch.inference_mode():
        mixed.st_buf = torch.zeros(7, 4, 16)
    mixed.stamp_constant_columns()
    assert mixed.const_stamp is None
    # normal tensors written in place under inference mode still move their counter: that write is seen
    seen = TrajSet(key=("normal",))
    seen.obs_buf, seen.st_buf = torch.zeros(4, 8, 16), None
    view = seen.obs_buf.permute(2, 0, 1)
    seen.stamp_constant_columns()
    with torch.inference_mode():
        assert seen.constant_columns_intact()
        view.mul_(2)
    assert not seen.constant_columns_intact()
