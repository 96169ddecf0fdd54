"""Guard-band tests of the forward entry points (``-m gpu``): every launch writes its outputs and nothing else.

Each case (tests/helpers_guard.py forward_rows(): the kernel forms of sim_plan.hpp row by row, at the smallest sizes at which each
has a ragged edge) runs the same call twice through the `_native` wrappers: plain, on ordinary torch tensors, and carved, with every
input, output and workspace a view of one 0xFF-filled arena, 64 KiB of untouched pattern on either side of each view. The carved
run is repeated per placement: everything at offset 0 modulo 256, then one argument group at a time (actions, observations, state
in / out, state trajectories, reward, terminated, truncated, references, workspace) at 16 and 48 (inside a 64-byte sector), 64
(16-byte aligned, not 128-byte aligned) and the element size — the pointers torch's allocator never hands out and sim_plan.hpp
decides on.

Per carved run:
(a) Arena.check(): every guard byte still 0xFF, every input bit-equal to its snapshot, no output element left at the pattern;
(b) where excenv_last_launch() names the same form as for the plain run, every output is torch.equal to the plain run's;
(c) where the placement made the planner pick another form, every output is held against the CPU oracle by the rule of
    tests/test_gpu_fuzz.py: identical bits for the trig-free models, else circ_close at 1e-9 (fp64) / 2e-5 (fp32) — observations,
    and the state trajectory and last state normalised to observation units, against the oracle's run; reward and flags against
    the oracle's on the states the launch itself wrote (flags equal), as tests/test_gpu_gym.py judges them;
(d) a call the library refuses must say so by code and name the alignment, and must have written nothing (check(wrote=False)).
At offset 0 the form must be the one the row was built to reach; the last test asserts that the forms seen cover every string
plan_name() can return and the four step_kernel names.

The trajectory, step and reward calls go to the C entry points with addresses (the argument order of `_native.sim_ahead_raw`,
`step_raw` and `rew_trunc_term`) instead of through those wrappers: the wrappers take tensors and pass `data_ptr()`, which torch
reports as NULL for an empty array (the reward rows of K = 0), and a carved view's address has to be the arena's own arithmetic,
base + offset, not something a wrapper derived. observe, state_from_observation, random_state, update_ref_to and update_ref go
through their wrappers.

No case hands the library a wrong size, pointer or stride: the arena only makes sure that a stray store of a correct call lands in
memory the test owns. A store more than 64 KiB away from every buffer of the call is not seen."""
import ctypes
import time

import numpy as np
import pytest
import torch

import oracle
from helpers import ANGLE_OBS, ANGLE_STATES, TRIG_FREE, circ_close, make_env
from helpers_forms import MODEL_CASES, SEM_ID, saturated_tables
from helpers_guard import (FORWARD_FORMS, HOLD_MAX, HOLD_MIN, Carved, Plain, arena_bytes, case_id, control_names, forward_rows,
                           guard_inputs, guard_spec, placements)

pytestmark = pytest.mark.gpu

ROWS = forward_rows()
SEEN = set()                       # every form a launch of this module reported
COUNTS = {}                        # entry point -> [runs, refusals]
LM, EM = 1, 0                      # EXCENV_LAYOUT_LANE_MAJOR, EXCENV_LAYOUT_ENV_MAJOR
EHIP = -3                          # EXCENV_EHIP: a launch failed; nothing more is started on the device after it


class Ctx:
    """One model on the device and as oracle properties"""

    def __init__(self, c):
        from helpers_lut import make_saturated

        env_name, _, lut = MODEL_CASES[c["model"]]
        self.env_name, self.dtype = env_name, getattr(torch, c["dtype"])
        self.names = control_names(env_name, c["controls"])
        B = c["B"]
        if lut is None:
            spec = guard_spec(c["model"], B, c["per_env"])
            self.env, self.oprops, self.keep, self.spec = make_env(env_name, B, self.dtype, c["solver"], spec=spec,
                                                                   control_state=list(self.names) or None)
        else:
            self.env, self.oprops, self.keep, self.spec = make_saturated(B, self.dtype, c["solver"], saturated_tables(c["model"]),
                                                                         control_state=list(self.names) or None)
        self.props, self.pkeep = self.env._props_for(self.env.env_properties, B)
        self.idx = [oracle.STATE_FIELDS[env_name].index(n) for n in self.names]
        self.S, self.A, self.O = len(oracle.STATE_FIELDS[env_name]), len(oracle.ACTION_FIELDS[env_name]), self.env._obs_dim() - len(self.names)


_CTX = {}


def ctx_of(c):
    key = (c["model"], c["solver"], c["dtype"], c["B"], c["controls"], c["per_env"])
    if key not in _CTX:
        if len(_CTX) > 8:
            _CTX.clear()
        _CTX[key] = Ctx(c)
    return _CTX[key]


def _control(ctx, alloc, names):
    from exciting_environments_amd import _native

    if not ctx.idx:
        return None
    ctl = _native.Control()
    ctl.n_control = len(ctx.idx)
    for j, f in enumerate(ctx.idx):
        ctl.control_idx[j] = f
        ctl.reference[j] = alloc.addr(names[j])
    return ctl


def _stream(ctx):
    from exciting_environments_amd import _native

    return _native._raw_stream(ctx.env.device)


def _check(rc, what):
    from exciting_environments_amd import _native

    if rc != 0:
        raise Refused(rc, _native.lib().excenv_last_error().decode("utf-8", "replace"), what)


class Refused(Exception):
    def __init__(self, rc, message, what):
        super().__init__(f"{what}: rc={rc}: {message}")
        self.rc, self.message = rc, message


def _ptrs(alloc, names):
    return (ctypes.c_void_p * len(names))(*[alloc.addr(n) for n in names])


# ---------------------------------------------------------------------------------------------------------------- the calls
def run_sim(ctx, c, inp, alloc):
    from exciting_environments_amd import _native

    env, dt = ctx.env, ctx.dtype
    S, A, O, nc = ctx.S, ctx.A, ctx.O, len(ctx.idx)
    B, K, sub = c["B"], c["K"], c["sub"]
    N, OW = K * sub, O + nc
    rows = N + 1
    lane_a, lane_t = c["a"] == "lane", c["t"] == "lane"
    out = {}
    sin = [f"state_in[{j}]" for j in range(S)]
    for j, n in enumerate(sin):
        alloc(n, (B,), dt, "state_io", fill=inp["st"][j])
    if K > 0:
        acts = inp["acts"]
        alloc("actions", (K, A, B) if lane_a else (B, K, A), dt, "actions", fill=np.ascontiguousarray(acts.transpose(1, 2, 0)) if lane_a else acts)
    rn = [f"reference[{j}]" for j in range(nc)]
    for j, n in enumerate(rn):
        alloc(n, (B,), dt, "refs", fill=inp["refs"][j])
    out["obs"] = alloc("obs_traj", (rows, OW, B) if lane_t else (B, rows, OW), dt, "obs", permute=(2, 0, 1) if lane_t else None)
    tn = [f"state_traj[{j}]" for j in range(S)] if c["states"] else None
    if tn:
        for j, n in enumerate(tn):
            out[n] = alloc(n, (rows, B) if lane_t else (B, rows), dt, "straj", permute=(1, 0) if lane_t else None)
    ln = [f"last_state[{j}]" for j in range(S)]
    for n in ln:
        out[n] = alloc(n, (B,), dt, "state_io")
    gym = None
    if c["gym"]:
        TW = _native.truncated_width(env.ENV_ID, nc)
        out["reward"] = alloc("reward", (N, B) if lane_t else (B, N), dt, "reward", permute=(1, 0) if lane_t else None)
        out["terminated"] = alloc("terminated", (N, B) if lane_t else (B, N), torch.bool, "terminated", permute=(1, 0) if lane_t else None)
        out["truncated"] = alloc("truncated", (rows, B, TW) if lane_t else (B, rows, TW), torch.bool, "truncated",
                                 permute=(1, 0, 2) if lane_t else None)
        gym = _native.TrajGym(alloc.addr("reward"), alloc.addr("terminated"), alloc.addr("truncated"))
    ws_bytes = 0
    if c["ws"]:
        ws_bytes = _native.sim_ahead_workspace_bytes(env.ENV_ID, dt, B, K, sub, nc, LM if lane_a else EM, LM if lane_t else EM, bool(tn))
        assert ws_bytes > 0
        alloc("workspace", (ws_bytes,), torch.uint8, "workspace", role="scratch")
    ctl = _control(ctx, alloc, rn)
    alloc.ready()
    tau = ctx.spec["tau"]
    _native.lib()
    for launch in range(2 if c["keep_twice"] else 1):  # keep_twice: the flag's promise holds from the second launch on
        flags = c["flags"] if (launch or not c["keep_twice"]) else 0
        opts = _native.launch_opts(c["epl"], c["emm"], 0, flags)
        with _native._on_device(env.device):
            rc = _native._lib.excenv_sim_ahead_ws(
                env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, K, sub, ctypes.byref(ctx.props), _native._ref(ctl), tau / sub, tau,
                _ptrs(alloc, sin), alloc.addr("actions") if K > 0 else None, LM if lane_a else EM, alloc.addr("obs_traj"),
                _ptrs(alloc, tn) if tn else None, LM if lane_t else EM, _ptrs(alloc, ln), SEM_ID[c["sem"]], _native._ref(gym),
                alloc.addr("workspace") if ws_bytes else None, ws_bytes, ctypes.byref(opts), _stream(ctx))
        _check(rc, "excenv_sim_ahead")
    return _native.last_launch(), out


def run_step(ctx, c, inp, alloc):
    from exciting_environments_amd import _native

    env, dt = ctx.env, ctx.dtype
    S, A, O, nc = ctx.S, ctx.A, ctx.O, len(ctx.idx)
    B = c["B"]
    out = {}
    sin, son = [f"state_in[{j}]" for j in range(S)], [f"state_out[{j}]" for j in range(S)]
    for j, n in enumerate(sin):
        alloc(n, (B,), dt, "state_io", fill=inp["st"][j])
    alloc("action", (B, A), dt, "actions", fill=np.ascontiguousarray(inp["acts"][:, 0]))
    rn = [f"reference[{j}]" for j in range(nc)]
    for j, n in enumerate(rn):
        alloc(n, (B,), dt, "refs", fill=inp["refs"][j])
    for n in son:
        out[n] = alloc(n, (B,), dt, "state_io")
    out["obs"] = alloc("obs", (B, O + nc), dt, "obs")
    gym = None
    if c["gym"]:
        TW = _native.truncated_width(env.ENV_ID, nc)
        out["reward"] = alloc("reward", (B,), dt, "reward")
        out["terminated"] = alloc("terminated", (B,), torch.bool, "terminated")
        out["truncated"] = alloc("truncated", (B, TW), torch.bool, "truncated")
        gym = (alloc.addr("reward"), alloc.addr("terminated"), alloc.addr("truncated"))
    ctl = _control(ctx, alloc, rn)
    alloc.ready()
    opts = _native.launch_opts(c["epl"])
    lib = _native.lib()
    args = [env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, ctypes.byref(ctx.props), _native._ref(ctl), ctx.spec["tau"], _ptrs(alloc, sin),
            alloc.addr("action"), _ptrs(alloc, son), alloc.addr("obs")]
    with _native._on_device(env.device):
        if gym is None:
            rc = lib.excenv_step(*args, ctypes.byref(opts), _stream(ctx))
        else:
            rc = lib.excenv_gym_step(*args, *gym, ctypes.byref(opts), _stream(ctx))
    _check(rc, "excenv_step")
    return _native.last_launch(), out


def run_rew(ctx, c, inp, alloc):
    from exciting_environments_amd import _native

    env, dt = ctx.env, ctx.dtype
    S, nc = ctx.S, len(ctx.idx)
    B, rows = c["B"], c["rows"]
    N = rows - 1
    in_lane, out_lane, vary = c["in_lane"], c["out_lane"], c["vary"]
    tn = [f"state_traj[{j}]" for j in range(S)]
    for j, n in enumerate(tn):
        leaf = inp["leaves"][j]
        alloc(n, (rows, B) if in_lane else (B, rows), dt, "straj", fill=np.ascontiguousarray(leaf.T) if in_lane else leaf)
    rn = [f"reference[{j}]" for j in range(nc)]
    strides = []
    for j, n in enumerate(rn):
        if vary:  # a reference per saved row, in the layout of the state leaves
            r = inp["row_refs"][j]
            alloc(n, (rows, B) if in_lane else (B, rows), dt, "refs", fill=np.ascontiguousarray(r.T) if in_lane else r)
            strides += [1, B] if in_lane else [rows, 1]
        else:
            alloc(n, (B,), dt, "refs", fill=inp["refs"][j])
            strides += [1, 0]
    TW = _native.truncated_width(env.ENV_ID, nc)
    out = {}
    if N > 0:
        out["reward"] = alloc("reward", (N, B) if out_lane else (B, N), dt, "reward", permute=(1, 0) if out_lane else None)
        out["terminated"] = alloc("terminated", (N, B) if out_lane else (B, N), torch.bool, "terminated", permute=(1, 0) if out_lane else None)
    out["truncated"] = alloc("truncated", (rows, B, TW) if out_lane else (B, rows, TW), torch.bool, "truncated",
                             permute=(1, 0, 2) if out_lane else None)
    ctl = _control(ctx, alloc, rn)
    alloc.ready()
    rs = (ctypes.c_int64 * len(strides))(*strides) if strides else None
    s_sb, s_sk = (1, B) if in_lane else (rows, 1)
    with _native._on_device(env.device):
        rc = _native.lib().excenv_rew_trunc_term(env.ENV_ID, _native.dtype_id(dt), B, rows, ctypes.byref(ctx.props), _native._ref(ctl), rs,
                                                 _ptrs(alloc, tn), s_sb, s_sk, alloc.addr("reward") if N > 0 else None,
                                                 alloc.addr("terminated") if N > 0 else None, alloc.addr("truncated"), LM if out_lane else EM,
                                                 _stream(ctx))
    _check(rc, "excenv_rew_trunc_term")
    return "traj_gym_kernel", out


def run_small(ctx, c, inp, alloc):
    """observe, state_from_observation, random_state, update_ref_to, update_ref through their `_native` wrappers"""
    from exciting_environments_amd import _native

    env, dt, kind = ctx.env, ctx.dtype, c["kind"]
    S, O, nc, B = ctx.S, ctx.O, len(ctx.idx), c["B"]
    out = {}
    if kind == "observe":
        st = [alloc(f"state[{j}]", (B,), dt, "state_io", fill=inp["st"][j]) for j in range(S)]
        rn = [f"reference[{j}]" for j in range(nc)]
        for j, n in enumerate(rn):
            alloc(n, (B,), dt, "refs", fill=inp["refs"][j])
        out["obs"] = alloc("obs", (B, O + nc), dt, "obs")
        ctl = _control(ctx, alloc, rn)
        alloc.ready()
        _native.observe(env.ENV_ID, dt, B, ctx.props, ctl, st, out["obs"])
    elif kind == "from_obs":
        obs = alloc("obs", (B, O + nc), dt, "obs", fill=inp["obs"])
        st = [alloc(f"state_out[{j}]", (B,), dt, "state_io") for j in range(S)]
        refs = [alloc(f"reference_out[{j}]", (B,), dt, "refs") for j in range(nc)]
        out.update({f"state_out[{j}]": t for j, t in enumerate(st)}, **{f"reference_out[{j}]": t for j, t in enumerate(refs)})
        alloc.ready()
        _native.state_from_observation(env.ENV_ID, dt, B, ctx.props, ctx.idx, obs, st, refs)
    elif kind == "random_state":
        keys = alloc("keys", (B, 2), torch.int64, "keys", fill=inp["keys"])
        st = [alloc(f"state_out[{j}]", (B,), dt, "state_io") for j in range(S)]
        leaf = alloc("key_leaf", (B, 2), torch.int64, "keys")
        out.update({f"state_out[{j}]": t for j, t in enumerate(st)}, key_leaf=leaf)
        alloc.ready()
        _native.random_state(env.ENV_ID, dt, B, ctx.props, keys, st, leaf)
    elif kind == "update_ref_to":
        rin = [alloc(f"reference_in[{j}]", (B,), dt, "refs", fill=inp["refs"][j]) for j in range(nc)]
        kin = alloc("keys_in", (B, 2), torch.int64, "keys", fill=inp["keys"])
        hin = alloc("hold_in", (B,), torch.int64, "keys", fill=inp["hold"])
        rout = [alloc(f"reference_out[{j}]", (B,), dt, "refs") for j in range(nc)]
        kout, hout = alloc("keys_out", (B, 2), torch.int64, "keys"), alloc("hold_out", (B,), torch.int64, "keys")
        out.update({f"reference_out[{j}]": t for j, t in enumerate(rout)}, keys_out=kout, hold_out=hout)
        alloc.ready()
        _native.update_ref_to(env.ENV_ID, dt, B, ctx.props, ctx.idx, rin, kin, hin, rout, kout, hout, HOLD_MIN, HOLD_MAX)
    else:  # update_ref: in place (the views are neither inputs that must stay nor outputs that must all change: "scratch")
        refs = [alloc(f"reference[{j}]", (B,), dt, "refs", fill=inp["refs"][j], role="scratch") for j in range(nc)]
        keys = alloc("keys", (B, 2), torch.int64, "keys", fill=inp["keys"], role="scratch")
        hold = alloc("hold", (B,), torch.int64, "keys", fill=inp["hold"], role="scratch")
        out.update({f"reference[{j}]": t for j, t in enumerate(refs)}, keys=keys, hold=hold)
        alloc.ready()
        _native.update_ref(env.ENV_ID, dt, B, ctx.props, ctx.idx, refs, keys, hold, HOLD_MIN, HOLD_MAX)
    return kind, out


def run_transpose(ctx, c, inp, alloc):
    from exciting_environments_amd import _native

    dt = getattr(torch, c["dtype"])
    M, N = c["M"], c["N"]
    x = alloc("in", (M, N), dt, "in", fill=inp["x"])
    y = alloc("out", (N, M), dt, "out")
    alloc.ready()
    _native._launch("excenv_transpose", x, "transpose", _native.dtype_id(dt), M, N, alloc.addr("in"), alloc.addr("out"))
    return "transpose", {"out": y}


RUN = {"sim": run_sim, "step": run_step, "rew": run_rew, "transpose": run_transpose}
ENTRY = {"sim": "excenv_sim_ahead_ws", "step": "excenv_step / excenv_gym_step", "rew": "excenv_rew_trunc_term", "observe": "excenv_observe",
         "from_obs": "excenv_state_from_observation", "random_state": "excenv_random_state", "update_ref_to": "excenv_update_ref_to",
         "update_ref": "excenv_update_ref", "transpose": "excenv_transpose"}


# ---------------------------------------------------------------------------------------------------------------- the oracle
_ORACLE = {}


def oracle_run(ctx, c, inp):
    """The CPU oracle's observations and state leaves of a sim / step case (computed once per case, on demand):
    dict(obs, states (S x [B, rows]) or None, last (S x [B]))"""
    key = case_id(c)
    if key not in _ORACLE:
        _ORACLE.clear()
        control = list(zip(ctx.names, inp["refs"]))
        tau = ctx.spec["tau"]
        if c["kind"] == "step":
            obs, last = oracle.step(ctx.env_name, c["solver"], inp["st"], inp["acts"][:, 0], ctx.oprops, tau, control=control)
            _ORACLE[key] = dict(obs=obs, states=None, last=last)
        else:
            obs, states, last = oracle.sim_ahead(ctx.env_name, c["solver"], inp["st"], inp["acts"], ctx.oprops, tau / c["sub"], env_tau=tau,
                                                 substeps=c["sub"], semantics=SEM_ID[c["sem"]], control=control)
            _ORACLE[key] = dict(obs=obs, states=states, last=last)
    return _ORACLE[key]


def close_to_oracle(ctx, got, want, angles):
    """tests/test_gpu_fuzz.py's rule on values in observation units: identical bits for the trig-free models, else circ_close at
    1e-9 (fp64) / 2e-5 (fp32), the columns `angles` on the circle of period 2"""
    if ctx.env_name in TRIG_FREE:
        return np.array_equal(got, want, equal_nan=True)
    tol = 1e-9 if ctx.dtype == torch.float64 else 2e-5
    return circ_close(got, want, angles, tol, tol)


def leaf_misses(ctx, j, got, want):
    """A state leaf against the oracle's by the same rule, in the units the rule is stated in: both are normalised with the
    field's range, (x - lo) / (hi - lo) * 2 - 1 in float64 (an observation column is exactly that), angle leaves on the circle."""
    if ctx.env_name in TRIG_FREE:
        return not np.array_equal(got, want)
    lo, hi = (np.asarray(v, dtype=np.float64) for v in ctx.spec["phys_norm"][oracle.STATE_FIELDS[ctx.env_name][j]])
    if got.ndim == 2:  # a per-environment bound [B] against a trajectory [B, rows]
        lo, hi = (v[:, None] if v.ndim == 1 else v for v in (lo, hi))
    norm = lambda x: ((np.asarray(x, dtype=np.float64) - lo) / (hi - lo) * 2 - 1)[..., None]
    return not close_to_oracle(ctx, norm(got), norm(want), [0] if j in ANGLE_STATES.get(ctx.env_name, []) else [])


def oracle_problems(ctx, c, inp, got):
    """(c): every output of a run whose form is not the plain run's, against the CPU oracle -> names of the outputs that miss.
    Observations, state trajectories and the last / new state against the oracle's run on the case's inputs; reward, terminated and
    truncated against the oracle's rew_trunc_term_ahead on the state trajectory this very launch wrote, as tests/test_gpu_gym.py
    judges the fused outputs (flags equal, reward by the rule above)."""
    want = oracle_run(ctx, c, inp)
    host = {n: t.cpu().numpy() for n, t in got.items()}
    bad = []
    if host["obs"].shape != want["obs"].shape or not close_to_oracle(ctx, host["obs"], want["obs"], ANGLE_OBS.get(ctx.env_name, [])):
        d = np.abs(host["obs"].astype(np.float64) - want["obs"]) if host["obs"].shape == want["obs"].shape and want["obs"].size else np.zeros(1)
        bad.append(f"obs (largest distance {float(np.nanmax(d)):.3e})")
    last = "state_out" if c["kind"] == "step" else "last_state"
    for j in range(ctx.S):
        if leaf_misses(ctx, j, host[f"{last}[{j}]"], want["last"][j]):
            bad.append(f"{last}[{j}]")
        if f"state_traj[{j}]" in host and leaf_misses(ctx, j, host[f"state_traj[{j}]"], want["states"][j]):
            bad.append(f"state_traj[{j}]")
    if c["gym"] and c["kind"] == "sim":
        own = [np.ascontiguousarray(host[f"state_traj[{j}]"]) for j in range(ctx.S)]  # every gym case stores its states
        rew, trunc, term = oracle.rew_trunc_term_ahead(ctx.env_name, own, ctx.oprops, control=list(zip(ctx.names, inp["refs"])))
        if not close_to_oracle(ctx, host["reward"], rew[..., 0], []):
            bad.append("reward")
        if not np.array_equal(host["terminated"], term[..., 0]):
            bad.append("terminated")
        if not np.array_equal(host["truncated"], trunc):
            bad.append("truncated")
    return bad


# ---------------------------------------------------------------------------------------------------------------- one case
def two_runs(c):
    """-> list of problems of one case over all its placements"""
    kind = c["kind"]
    run = RUN.get(kind, run_small)
    cid = case_id(c)
    if kind == "transpose":
        ctx = None
        inp = dict(x=np.random.default_rng(3).uniform(-1, 1, (c["M"], c["N"])).astype(c["dtype"]))
    else:
        ctx = ctx_of(c)
        inp = guard_inputs(ctx.env_name, ctx.spec, c["dtype"], c["B"], 1 if kind == "step" else c["K"], ctx.names, rows=c.get("rows", 0))
    count = COUNTS.setdefault(ENTRY[kind], [0, 0])
    plain = Plain()
    form0, ref = run(ctx, c, inp, plain)
    torch.cuda.synchronize()
    SEEN.add(form0)
    problems = []
    if c["expect"] is not None and form0 != c["expect"]:
        problems.append(f"{cid}: plain run launched {form0!r}, the row was built to reach {c['expect']!r}")
    size = arena_bytes(plain.sizes)
    for place in placements(c, c["sweep"], c["extra"]):
        where = f"{cid} @ {place or 'offset 0'}"
        carved = Carved(size, place)
        count[0] += 1
        try:
            form, got = run(ctx, c, inp, carved)
        except (Refused, RuntimeError) as e:  # (d): refused by code, the alignment named, nothing written
            torch.cuda.synchronize()
            count[1] += 1
            print(f"guard {where}: plain {form0!r}, carved refused: {e}")
            msg = str(e)
            if getattr(e, "rc", -1) == EHIP or "rc=-3" in msg or "HIP error" in msg:
                pytest.exit(f"guard {where}: the GPU reported a fault, nothing more is launched: {msg}", returncode=3)
            if not place or "align" not in msg or "rc=-1" not in msg:
                problems.append(f"{where}: refused without naming the alignment: {msg}")
            problems += [f"{where}: {p}" for p in carved.arena.problems(wrote=False)]
            continue
        torch.cuda.synchronize()
        SEEN.add(form)
        print(f"guard {where}: plain {form0!r}, carved {form!r}")
        if not place and c["expect"] is not None and form != c["expect"]:
            problems.append(f"{where}: launched {form!r}, the row was built to reach {c['expect']!r}")
        problems += [f"{where} [{form}]: {p}" for p in carved.arena.problems()]                                  # (a)
        if form == form0:                                                                                        # (b)
            bad = [n for n in ref if not torch.equal(got[n], ref[n])]
            if bad:
                problems.append(f"{where} [{form}]: {bad} differ from the plain run of the same form")
        else:                                                                                                    # (c)
            bad = oracle_problems(ctx, c, inp, got)
            if bad:
                problems.append(f"{where} [{form} instead of {form0}]: {bad} miss the oracle bound")
    for p in problems:
        print("guard problem:", p)
    return problems


def _params(row, size=12):
    """The cases of a row in chunks: one pytest case each, a few seconds at the most"""
    cases = ROWS[row]
    return [pytest.param(cases[i:i + size], id=f"{row}-{i // size:02d}") for i in range(0, len(cases), size)]


ALL = [p for row, size in (("step", 20), ("general", 8), ("lean", 12), ("lean_gym", 6), ("control_fill", 8), ("aem", 6), ("em", 15),
                           ("emr", 8), ("workspace", 6), ("row_sync", 1), ("wide", 1), ("saturated", 6), ("rew", 36), ("small", 36),
                           ("transpose", 8)) for p in _params(row, size)]
TIMES = []


@pytest.mark.parametrize("cases", ALL)
def test_every_launch_writes_its_outputs_and_nothing_else(cases):
    t0 = time.perf_counter()
    problems = []
    try:
        for c in cases:
            problems += two_runs(c)
    except RuntimeError as e:  # a fault the device reports at a synchronisation: the run stops here
        pytest.exit(f"guard forward: {e}", returncode=3)
    TIMES.append(time.perf_counter() - t0)
    assert not problems, "\n".join(problems[:40]) + (f"\n... {len(problems) - 40} more" if len(problems) > 40 else "")


def test_every_named_form_was_reached():
    """A planner change that silently stops a form from being reached fails here instead of shrinking the sweep. Depends on the
    order of the file: it reads what the cases above recorded in this process, so it has to run after them (pytest's default
    order; under a selection or a reordering plugin it skips and says so)."""
    print("guard forward: (form, size, placement) runs and refusals per entry point:",
          {k: f"{v[0]} runs, {v[1]} refused" for k, v in sorted(COUNTS.items())})
    print(f"guard forward: {sum(TIMES):.1f} s in {len(TIMES)} cases, slowest {max(TIMES, default=0.0):.1f} s")
    print("guard forward: forms reached:", sorted(SEEN))
    if len(TIMES) < len(ALL):
        pytest.skip("only a selection of this module's cases ran: the form list is judged over the whole module")
    missing = [f for f in FORWARD_FORMS if f not in SEEN]
    assert not missing, f"forms never launched: {missing}"
