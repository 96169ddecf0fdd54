"""The guard-band arena of tests/helpers_guard.py on the CPU (no GPU): the checker must be able to fail, the carved views must have
the properties the GPU tests rely on, and the condition behind "no output element still holds the all-ones pattern" must hold for
every case of tests/test_gpu_guard_forward.py and tests/test_gpu_guard_reverse.py: a correct launch on these inputs stores finite
numbers and flags that are 0 or 1."""
import numpy as np
import pytest
import torch

import oracle
from helpers_forms import MODEL_CASES, SEM_ID
from helpers_guard import (FORWARD_FORMS, GUARD, HOLD_MAX, HOLD_MIN, PATTERN, Arena, Carved, GuardError, Plain, arena_bytes, case_id,
                           control_names, forward_rows, groups_of, guard_inputs, guard_spec, placements, saturated_host_spec)

DTYPES = [torch.float32, torch.float64, torch.int64, torch.bool, torch.uint8]


def _arena():
    """A CPU arena the way a GPU case builds one: two inputs, two outputs (one strided), a workspace"""
    a = Arena(arena_bytes([4 * 65, 8 * 7, 4 * 3 * 2 * 65, 65 * 3, 1000]), "cpu")
    x = a.carve((65,), torch.float32, 16, "in", "state_in[0]")
    k = a.carve((7,), torch.int64, 8, "in", "keys")
    obs = a.carve((3, 2, 65), torch.float32, 48, "out", "obs_traj", permute=(2, 0, 1))
    flags = a.carve((65, 3), torch.bool, 1, "out", "truncated")
    ws = a.carve((1000,), torch.uint8, 64, "scratch", "workspace")
    x.copy_(torch.arange(65, dtype=torch.float32))
    k.copy_(torch.arange(7))
    a.seal()
    return a, x, k, obs, flags, ws


def _launch(obs, flags):
    """What a correct launch does: every output element written with finite values / 0-1 flags"""
    obs.copy_(torch.rand(obs.shape))
    flags.copy_(torch.rand(flags.shape) < 0.5)


# ------------------------------------------------------------------------------------------------ 1: the checker can fail
def test_a_correct_launch_passes_and_an_idle_one_is_seen_as_refused():
    a, x, k, obs, flags, ws = _arena()
    a.check(wrote=False)  # nothing ran: what a refused call must leave behind
    with pytest.raises(GuardError, match="'obs_traj' not written: 390 of 390"):
        a.check()
    _launch(obs, flags)
    ws[:10] = 0  # a workspace may be written anywhere inside itself
    a.check()
    with pytest.raises(GuardError, match="'obs_traj' written by a refused call"):
        a.check(wrote=False)


def test_one_flipped_guard_byte_is_reported_with_both_neighbours():
    a, x, k, obs, flags, ws = _arena()
    _launch(obs, flags)
    v = {w.name: w for w in a.views}
    # one byte behind the observations (a tail lane's store), then one in front of the flags: two different guards
    a.buf[v["obs_traj"].start + v["obs_traj"].nbytes + 3] = 0
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert "guard damaged: 1 bytes" in msg and "between 'obs_traj' and 'truncated'" in msg and "3 bytes behind 'obs_traj'" in msg
    a.buf[v["truncated"].start - 1] = 7
    msg = "; ".join(a.problems())
    assert "guard damaged: 2 bytes" in msg and "1 bytes in front of 'truncated'" not in msg.split("last at")[0]
    assert msg.count("between 'obs_traj' and 'truncated'") == 2
    # the first and the last byte of the whole arena are guards too
    a.buf[v["truncated"].start - 1] = PATTERN
    a.buf[v["obs_traj"].start + v["obs_traj"].nbytes + 3] = PATTERN
    a.check()
    a.buf[0] = 0
    assert "between None and 'state_in[0]'" in "; ".join(a.problems())
    a.buf[0] = PATTERN
    a.buf[-1] = 0
    assert "between 'workspace' and None" in "; ".join(a.problems())


def test_one_unwritten_output_element_is_reported_by_view_name():
    a, x, k, obs, flags, ws = _arena()
    _launch(obs, flags)
    obs[64, 2, 1] = torch.tensor(float("nan")).view(torch.int32).fill_(-1).view(torch.float32)  # all-ones: left as the arena made it
    with pytest.raises(GuardError, match=r"output 'obs_traj' not written: 1 of 390 elements, first at element 389"):
        a.check()
    obs[64, 2, 1] = 0.5
    a.check()
    flags.view(torch.uint8)[10, 1] = 255
    with pytest.raises(GuardError, match=r"output 'truncated' not written: 1 of 195 elements, first at element 31"):
        a.check()


def test_one_changed_input_element_is_reported_by_view_name():
    a, x, k, obs, flags, ws = _arena()
    _launch(obs, flags)
    x[5] += 1.0
    with pytest.raises(GuardError, match=r"input 'state_in\[0\]' changed"):
        a.check()
    x[5] -= 1.0
    a.check()
    k[6] = -1
    with pytest.raises(GuardError, match=r"input 'keys' changed: 8 bytes, first at byte 48, last at byte 55"):
        a.check()


def test_zero_filled_outputs_are_checked_for_zeros():
    a = Arena(arena_bytes([40, 40]), "cpu")
    g = a.carve((10,), torch.float32, 0, "out", "grad[0]")
    z = a.carve((10,), torch.float32, 0, "out", "grad[1]")
    a.seal()
    g.fill_(1.0)
    z.zero_()
    a.check(zero_filled=("grad[1]",))
    z[3] = 1e-30
    with pytest.raises(GuardError, match=r"output 'grad\[1\]' not zero-filled: [1-4] bytes, first at byte 1[2-5]"):
        a.check(zero_filled=("grad[1]",))


# ------------------------------------------------------------------------------------------------ 2: the carve properties
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_offsets_are_honoured_for_every_dtype(dtype):
    isz = torch.empty((), dtype=dtype).element_size()
    offsets = sorted({0, 16, 48, 64, 128, isz, 256 - isz} | ({1, 2, 4} if isz == 1 else set()))
    a = Arena(arena_bytes([isz * 37] * len(offsets)), "cpu")
    for off in offsets:
        t = a.carve((37,), dtype, off, "out", f"v{off}")
        assert t.data_ptr() % 256 == off and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == (37,)
    with pytest.raises(AssertionError):
        a.carve((3,), torch.float64, 4, "out", "misaligned element")


def test_no_two_views_or_guards_overlap_and_every_byte_is_pattern():
    a, *_ = _arena()
    assert bool((Arena(1000, "cpu").buf == PATTERN).all())
    spans = [(v.start, v.start + v.nbytes) for v in a.views]
    for (s0, e0), (s1, e1) in zip(spans, spans[1:]):
        assert s1 - e0 >= 2 * GUARD  # the guard behind one view and the guard in front of the next are different bytes
    assert spans[0][0] >= GUARD and a.buf.numel() - spans[-1][1] >= GUARD
    ranges = a.guard_ranges()
    assert ranges[0][0] == 0 and ranges[-1][1] == a.buf.numel()
    covered = sum(b - s for s, b, _, _ in ranges) + sum(e - s for s, e in spans)
    assert covered == a.buf.numel()  # guards and views tile the arena
    assert int(a.guard_mask.sum()) == a.buf.numel() - sum(e - s for s, e in spans)
    with pytest.raises(MemoryError):
        a.sealed = False
        a.carve((1 << 20,), torch.float32, 0, "out", "too large")


def test_strided_views_address_only_their_own_bytes():
    a = Arena(arena_bytes([8 * 4 * 3 * 5, 4 * 6 * 5]), "cpu")
    obs = a.carve((4, 3, 5), torch.float64, 16, "out", "obs", permute=(2, 0, 1))   # [rows][OW][B] seen as [B, rows, OW]
    leaf = a.carve((6, 5), torch.float32, 4, "out", "leaf", permute=(1, 0))        # [rows][B] seen as [B, rows]
    assert tuple(obs.shape) == (5, 4, 3) and tuple(obs.stride()) == (1, 15, 5)
    assert tuple(leaf.shape) == (5, 6) and tuple(leaf.stride()) == (1, 5)
    a.seal()
    obs.fill_(2.0)
    leaf.fill_(3.0)
    a.check()  # every element of both blocks written through the strided views, no guard byte touched
    for v, t in zip(a.views, (obs, leaf)):
        lo = t.data_ptr() - a.base
        hi = lo + (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()
        assert (lo, hi) == (v.start, v.start + v.nbytes)


def test_the_two_providers_hand_out_the_same_buffers():
    """Plain and Carved take the same calls; the arena is sized from what the plain run asked for; empty arrays have an address"""
    def ask(alloc):
        x = alloc("x", (5, 2), torch.float32, "actions", fill=np.arange(10, dtype=np.float32).reshape(5, 2))
        y = alloc("y", (2, 5), torch.float64, "obs", permute=(1, 0))
        e = alloc("empty", (0, 5), torch.float32, "reward")
        s = alloc("s", (3,), torch.int64, "keys", fill=np.arange(3), role="scratch")
        alloc.ready()
        return x, y, e, s

    plain = Plain("cpu")
    px = ask(plain)
    carved = Carved(arena_bytes(plain.sizes), {"obs": 48, "keys": 8}, "cpu")
    cx = ask(carved)
    for p, c in zip(px, cx):
        assert p.shape == c.shape and p.dtype == c.dtype and p.stride() == c.stride()
    assert torch.equal(px[0], cx[0]) and torch.equal(px[3], cx[3])
    assert carved.addr("y") % 256 == 48 and carved.addr("s") % 256 == 8 and carved.addr("x") % 256 == 0
    assert carved.addr("y") == cx[1].data_ptr() and plain.addr("x") == px[0].data_ptr()
    assert plain.addr("empty") != 0 and carved.addr("empty") != 0
    assert [v.role for v in carved.arena.views] == ["in", "out", "out", "scratch"]
    cx[1].fill_(1.0)
    carved.arena.check()


# ------------------------------------------------------------------------------------------------ 3: everything written is not the pattern
def test_placements_move_one_group_at_a_time():
    c = forward_rows()["lean_gym"][0]
    ps = placements(c, "full")
    assert ps[0] == {} and all(len(p) == 1 for p in ps[1:])
    assert {g for p in ps[1:] for g in p} == set(groups_of(c)) == {"actions", "obs", "state_io", "straj", "reward", "terminated", "truncated"}
    assert {o for p in ps[1:] for g, o in p.items() if g == "obs"} == {16, 48, 64, 4}
    assert {o for p in ps[1:] for g, o in p.items() if g == "truncated"} == {16, 48, 64, 4, 2, 1}
    small = {c["kind"]: groups_of(c) for c in forward_rows()["small"] if c["controls"] or c["kind"] == "random_state"}  # what the call has
    assert small == {"observe": ["state_io", "obs", "refs"], "from_obs": ["obs", "state_io", "refs"], "random_state": ["keys", "state_io"],
                     "update_ref_to": ["refs", "keys"], "update_ref": ["refs", "keys"]}
    assert all("refs" not in groups_of(c) for c in forward_rows()["small"] if not c["controls"])
    ids = [case_id(c) for r in forward_rows().values() for c in r]
    assert len(ids) == len(set(ids))
    expected = {c["expect"] for r in forward_rows().values() for c in r if c["expect"]}
    assert expected == set(FORWARD_FORMS)  # the rows are built to reach every named form


def _host_model(c):
    env_name, _, lut = MODEL_CASES[c["model"]]
    npdt = np.dtype(c["dtype"]).type
    if lut is None:
        spec = guard_spec(c["model"], c["B"], c["per_env"])
        props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], npdt, c["B"])
    else:
        spec, prepared = saturated_host_spec(c["model"])
        props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], npdt, c["B"], pmsm_lut=prepared)
    return env_name, spec, props, keep


def _finite(what, *arrays):
    for a in arrays:
        a = np.asarray(a)
        assert a.size == 0 or bool(np.isfinite(a).all()), what


@pytest.mark.parametrize("row", list(forward_rows()))
def test_the_oracle_is_finite_on_every_forward_case(row):
    """One oracle run per distinct (model, inputs, call): placements and launch shaping do not change what a correct launch stores"""
    done = set()
    for c in forward_rows()[row]:
        kind = c["kind"]
        if kind == "transpose":
            continue  # uniform numbers in, the same numbers out
        key = (kind, c["model"], c["solver"], c["dtype"], c["B"], c["K"], c["sub"], c["sem"], c["controls"], c["per_env"], c["gym"], c.get("rows"),
               c.get("vary"))
        if key in done:
            continue
        done.add(key)
        env_name, spec, props, keep = _host_model(c)
        names = control_names(env_name, c["controls"])
        inp = guard_inputs(env_name, spec, c["dtype"], c["B"], 1 if kind == "step" else c["K"], names, rows=c.get("rows", 0))
        control = list(zip(names, inp["refs"]))
        where = case_id(c)
        tau = spec["tau"]
        _finite(where, *inp["st"], inp["acts"], *inp["refs"])
        if kind == "step":
            obs, st, rew, term, trunc = oracle.gym_step(env_name, c["solver"], inp["st"], inp["acts"][:, 0], props, tau, control=control)
            _finite(where, obs, *st, rew)
        elif kind == "sim":
            obs, straj, last = oracle.sim_ahead(env_name, c["solver"], inp["st"], inp["acts"], props, tau / c["sub"], env_tau=tau,
                                                substeps=c["sub"], semantics=SEM_ID[c["sem"]], control=control)
            _finite(where, obs, *straj, *last)
            if c["gym"]:
                rew, trunc, term = oracle.rew_trunc_term_ahead(env_name, straj, props, control=control)
                _finite(where, rew)
        elif kind == "rew":
            _finite(where, *inp["leaves"], *inp["row_refs"])
            if c["vary"]:  # a reference per row: every (environment, row) is an environment of its own with two equal rows
                flat = [np.repeat(l.reshape(-1, 1), 2, axis=1) for l in inp["leaves"]]
                fp, fkeep = _host_model(dict(c, B=c["B"] * c["rows"]))[2:]
                rew, trunc, term = oracle.rew_trunc_term_ahead(env_name, flat, fp,
                                                               control=[(n, r.reshape(-1)) for n, r in zip(names, inp["row_refs"])])
            else:
                rew, trunc, term = oracle.rew_trunc_term_ahead(env_name, inp["leaves"], props, control=control)
            _finite(where, rew)
        elif kind in ("observe", "from_obs"):
            obs = oracle.sim_ahead(env_name, "euler", inp["st"], inp["acts"][:, :0], props, tau, control=control)[0]
            _finite(where, obs)
            if kind == "from_obs":
                box = {n: tuple(np.asarray(v, dtype=np.float64) for v in spec["phys_norm"][n]) for n in spec["phys_norm"]}
                own = inp["obs"][:, :obs.shape[-1] - len(names)].astype(np.float64)
                _finite(where, inp["obs"], *oracle.state_from_observation(env_name, own, box))
        elif kind == "random_state":
            st, leaf = oracle.random_state(env_name, inp["keys"], props, np.dtype(c["dtype"]))
            _finite(where, *st)
            assert bool((leaf >= 0).all()) and bool((inp["keys"] >= 0).all()), where  # uint32 words in int64: never -1
        else:  # update_ref_to / update_ref
            idx = [oracle.STATE_FIELDS[env_name].index(n) for n in names]
            refs, keys, hold = oracle.update_ref(env_name, idx, inp["refs"], inp["keys"], inp["hold"], props, np.dtype(c["dtype"]), HOLD_MIN,
                                                 HOLD_MAX)
            _finite(where, *refs)
            assert bool((keys >= 0).all()) and bool((hold >= 0).all()), where
            assert c["B"] == 1 or (bool((inp["hold"] == 0).any()) and bool((inp["hold"] > 0).any())), where  # due and not due
        if kind in ("step", "sim", "rew") and (c["gym"] or kind == "rew"):
            for flags in (term, trunc):
                assert set(np.unique(np.asarray(flags).astype(np.uint8))) <= {0, 1}, where


# ---- the reverse cases: the references are finite on the inputs the carved runs use (tests/test_gpu_guard_reverse.py)
def _rev_input_sets():
    """One case per distinct (input arrays, solver, semantics) of rev_sim_cases(): V = 1 at B = 1 and 257, the wide B = V * 326"""
    from helpers_guard import rev_sim_cases

    seen, out = set(), []
    for c in rev_sim_cases() + rev_sim_cases(True):
        key = (c["env"], c["deadtime"], c["elem"], c["B"], c["sub"], c["wide"], c["solver"], c["sem"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_the_twin_is_finite_on_the_reverse_trajectory_inputs():
    from helpers_guard import rev_sim_inputs
    from helpers_vjp import Twin, vjp

    for c in _rev_input_sets():
        spec, st, acts, (g_obs, g_states, g_last) = rev_sim_inputs(c)
        _finite(c, *st, acts, g_obs, *g_states, *g_last)
        twin = Twin(c["env"], spec, c["solver"], c["sem"])
        ga, gs, _ = vjp(twin, [v.astype(np.float64) for v in st], acts.astype(np.float64), spec["tau"], c["sub"], g_obs=g_obs,
                        g_states=g_states, g_last=g_last)
        _finite(c, ga, *gs)


def test_the_references_are_finite_on_the_step_reward_and_feedback_inputs():
    from conftest import ENV_NAMES
    from helpers_feedback import CLIP, feedback_inputs, oracle_closed_loop, substeps_of
    from helpers_reward_vjp import ROWS, control_sets, oracle_grads, reward_inputs, wide_b
    from helpers_step_vjp import CONTROL, refs_for, step_inputs, twin_step, twin_step_grads
    from helpers_vjp import CASES, skewed_spec

    for env_name, deadtime in CASES:
        for B in (1, 193, 257):  # excenv_step_vjp, excenv_step_jacobian (its rows are these steps' one-hot cotangents)
            spec, st, act = step_inputs(env_name, deadtime, B)
            control = CONTROL[env_name]
            refs = refs_for(env_name, control, spec, B)
            tw = twin_step(env_name, spec, "rk4", st, act, control, refs)
            rng = np.random.default_rng(B)
            ga, gs = twin_step_grads(tw, rng.normal(size=(B, tw[2].shape[1])), [rng.normal(size=B) for _ in st], rng.normal(size=B))
            _finite((env_name, B), *st, act, ga, *gs, tw[2].detach().numpy(), *[x.detach().numpy() for x in tw[3]])
        spec = skewed_spec(env_name, deadtime)
        for B, K in ((1, 7), (326, 0), (326, 1), (326, 7)):  # excenv_sim_feedback
            for per_env in (True, False):
                inp = feedback_inputs(env_name, spec, B, K, per_env_gains=per_env)
                props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
                res = oracle_closed_loop(env_name, "rk4", props, inp, spec["tau"], K=K, sub=substeps_of(env_name), clip=CLIP)
                _finite((env_name, B, K, per_env), res["obs"], *res["states"], *res["last"], res["actions"], res["z"])
    for env_name in ENV_NAMES:  # excenv_rew_vjp
        sets = [s for s in control_sets(env_name) if s]
        for control in (sets[0], sets[-1]):
            for B in (wide_b(4), wide_b(8), 257):
                data = reward_inputs(env_name, control, B, ROWS, 8)
                grads = oracle_grads(env_name, control, data["leaves"], data["refs"], data["g"])
                _finite((env_name, control, B), *data["leaves"], *data["refs"].values(), data["g"], *[g for g in grads if g is not None])


# ---- what excenv_last_launch() cannot tell: the rows of the table that share a name (sim_plan.hpp through tests/test_sim_plan.py's driver)
def test_the_planner_takes_the_paths_the_cases_are_built_for(tmp_path):
    """Both row_sync paths report "sim_ahead_kernel (V=1)", and a width that steps down reports only the narrower name: the planner
    itself, compiled for the host, must give row_sync 2 (rows through LDS) for the row_sync cases of whole workgroups at 16-byte
    aligned placements, 1 (barrier rows) for the ragged batch and for a trajectory array at the element size, and the stepped-down
    width for B = 1302 and 1301. A planner change that moves ROW_SYNC_MIN_BATCH past the test sizes fails here."""
    import subprocess

    from test_sim_plan import CSRC, CXX, DRIVER, FIELDS, SOLVERS, facts
    from helpers_guard import ELEM, fallen_width

    assert CXX is not None, "no host C++ compiler"
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    al = lambda off: 128 if off % 128 == 0 else (off & -off)
    asked = []
    for c in forward_rows()["row_sync"] + [c for c in forward_rows()["lean"] if c["B"] in (1300, 1301, 1302)]:
        for place in placements(c, c["sweep"], c["extra"]):
            f = facts(MODEL_CASES[c["model"]][0], ELEM[c["dtype"]], c["solver"], B=c["B"], K=c["K"], substeps=c["sub"], semantics=SEM_ID[c["sem"]],
                      state_traj=c["states"], envs_per_lane=c["epl"], al_obs=al(place.get("obs", 0)), al_straj=al(place.get("straj", 0)),
                      al_actions=al(place.get("actions", 0)), al_state_io=al(place.get("state_io", 0)))
            asked.append((c, place, f))
    out = subprocess.run([str(exe)], input="\n".join(" ".join(str(f[n]) for n in FIELDS) for _, _, f in asked) + "\n", capture_output=True,
                         text=True, check=True).stdout.splitlines()
    assert len(out) == len(asked)
    seen = set()
    for (c, place, f), line in zip(asked, out):
        nums, name = line.split("|")
        form, ws, V, threads, row_sync, row_lds, split, period, inst = map(int, nums.split())
        vector = all(o % 16 == 0 for o in place.values())
        if c["B"] >= 1 << 17:
            want = 2 if (c["B"] % 256 == 0 and vector) else 1
            assert (row_sync, V, name) == (want, 1, c["expect"]), (case_id(c), place)
            assert (row_lds > 0) == (want == 2) and row_lds <= GUARD
            seen.add(want)
        else:
            assert row_sync == 0 and V == (fallen_width(c["epl"], c["B"]) if vector else 1), (case_id(c), place)
            assert place or name == c["expect"]
            seen.add((c["epl"], V))
    assert {1, 2} <= seen and {(4, 2), (4, 1), (2, 1), (4, 4)} <= seen
