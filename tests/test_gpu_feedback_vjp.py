"""Reverse mode of the closed loop on the GPU (`vmap_sim_ahead_feedback_vjp`, `vmap_sim_ahead_feedback(differentiable=True)`;
sim_feedback_vjp_kernel, feedback_z_rows_kernel, feedback_gain_grad_kernel):
1. fp64 against the float64 torch twin (helpers_feedback_vjp): every model, three solvers, the full policy, four cotangent groups,
   every returned gradient within 1e-8 of the twin's relative to the tensor's largest magnitude;
2. against the parent commit's own code: the same loop as a chain of differentiable vmap_step calls with the policy in torch, 2e-8;
3. fp32: within 32 x the forward floor, environments inside KINK_MARGIN excluded (their share <= KINK_CAP);
4. the pre-pass: its last row is the forward's returned z, bit for bit;
5. forms: broadcast / per-environment / mixed gains, control columns, no feedforward / integrator / clamp, K = 1, B = 1, K = 0;
6. zero gains: the open-loop reverse kernel on the returned actions;
7. the recording form;
8. a directional finite difference in fp64;
9. guard bands around every buffer of the three launches.
Every case prints its figures."""
import ctypes

import numpy as np
import pytest
import torch

import helpers_feedback as hf
import helpers_feedback_vjp as hv
import oracle
from exciting_environments_amd import _native
from helpers import NP_DTYPE, make_env, to_state
from helpers_vjp import KINK_CAP, KINK_MARGIN, case_spec, obs_floor, rel_dist

pytestmark = pytest.mark.gpu
TOL = 1e-8


def _dev(x, env):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=env.dtype, device=env.device)


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def rounded(inp, dtype):
    """The inputs as the kernel sees them: rounded to the working dtype, as float64"""
    npdt = NP_DTYPE[dtype]
    r = lambda v: None if v is None else np.asarray(v).astype(npdt).astype(np.float64)
    out = {k: r(inp[k]) for k in ("gain", "igain", "ff", "z0")}
    out["st"] = [r(v) for v in inp["st"]]
    out["refs"] = None if inp.get("refs") is None else {n: r(v) for n, v in inp["refs"].items()}
    return out


def forward(env, inp, K, sub, tau, clip=hf.CLIP, control=None, **kw):
    """One vmap_sim_ahead_feedback call -> dict of its arguments and what it returned"""
    state = to_state(env, inp["st"], reference=inp["refs"] if control else None)
    a = dict(gain=_dev(inp["gain"], env), ff=_dev(inp["ff"], env), igain=_dev(inp["igain"], env), z0=_dev(inp["z0"], env))
    obs, states, last, actions, z = env.vmap_sim_ahead_feedback(state, a["gain"], K, tau, tau * sub, feedforward=a["ff"],
                                                                integral_gain=a["igain"], integrator_state=a["z0"], clip=clip, **kw)
    return dict(env=env, state=state, obs=obs, states=states, last=last, actions=actions, z=z, K=K, sub=sub, tau=tau, clip=clip, **a)


def explicit(run, group):
    """vmap_sim_ahead_feedback_vjp on a forward run for one cotangent group (helpers_feedback_vjp.cotangent_groups) -> dict of float64
    numpy gradients named like the twin's"""
    env = run["env"]
    d = lambda v: None if v is None else _dev(v, env)
    dl = lambda vs: None if vs is None else [d(v) for v in vs]
    gs, gg, ggi, gff, gz0 = env.vmap_sim_ahead_feedback_vjp(
        run["state"], run["gain"], run["obs"], run["states"], run["actions"], run["tau"], run["tau"] * run["sub"],
        integral_gain=run["igain"], integrator_state=run["z0"], clip=run["clip"], grad_obs=d(group.get("obs")),
        grad_states=dl(group.get("states")), grad_last_state=dl(group.get("last")),
        grad_actions=d(group.get("actions")) if run["K"] > 0 else None, grad_z=d(group.get("z")))
    assert env.last_feedback_vjp_launch == "sim_feedback_vjp_kernel", env.last_feedback_vjp_launch
    torch.cuda.synchronize()
    return dict(state0=[_np(getattr(gs, n)) for n in env.STATE_FIELDS], gain=_np(gg), igain=_np(ggi), ff=_np(gff), z0=_np(gz0),
                raw=(gs, gg, ggi, gff, gz0))


def compare(got, want, keep=None, per_env=True):
    """-> {name: relative distance} of every gradient both sides have (keep: environments compared, for per-environment tensors)"""
    out = {}
    for j, (g, w) in enumerate(zip(got["state0"], want["state0"])):
        out[f"state0[{j}]"] = rel_dist(g, w, keep)
    for n in ("gain", "igain", "ff", "z0"):
        if want[n] is None:
            assert got[n] is None, n
            continue
        k = keep if (per_env or n in ("ff", "z0")) else None
        out[n] = rel_dist(got[n], want[n], k)
    return out


def check(dist, bound, label):
    worst = max(dist.values())
    print(f"{label}: worst {worst:.3e} (bound {bound:.3e}) " + " ".join(f"{k}={v:.2e}" for k, v in dist.items()))
    assert worst <= bound, (label, dist)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("solver", hf.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hf.CASES)
def test_fp64_gradients_equal_the_twins(env_name, deadtime, solver):
    spec, inp, twin, lv, out = hv.main_twin(env_name, deadtime, solver)
    K, sub = hf.K_MAIN, hf.substeps_of(env_name)
    env, _, _, _ = make_env(env_name, hf.B_MAIN, torch.float64, solver, spec=spec)
    run = forward(env, inp, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    groups = hv.cotangent_groups(np.random.default_rng(5), hf.B_MAIN, K * sub + 1, OW, S, K, A)
    want = hv.twin_grads(lv, out, groups, OW)
    names = ("all", "last_state", "obs", "actions+z")
    seen = []
    for name, group, w in zip(names, groups, want):
        got = explicit(run, group)
        seen.append(dict(env.last_feedback_vjp_cotangents))
        check(compare(got, w), TOL, f"{env_name} dead={deadtime} {solver} [{name}]")
    assert seen[0] == dict(obs=True, states=[True] * S, last_state=[True] * S, actions=True, z=True)
    assert seen[1] == dict(obs=False, states=[False] * S, last_state=[True] * S, actions=False, z=False)
    assert seen[2]["obs"] and not seen[2]["actions"] and seen[3] == dict(obs=False, states=[False] * S, last_state=[False] * S, actions=True, z=True)


# ---------------------------------------------------------------------------------------------------------------- 2
def _torch_policy(ob, gain, igain, ff_k, z, lo, hi, adt):
    """The policy in torch, torch.where masks with strict comparisons, the sums as addcmul in column order"""
    acc = ff_k + z
    zi = torch.zeros_like(z)
    for o in range(ob.shape[1]):
        acc = torch.addcmul(acc, gain[:, :, o], ob[:, o:o + 1])
        zi = torch.addcmul(zi, igain[:, :, o], ob[:, o:o + 1])
    a = torch.where((acc > lo) & (acc < hi), acc, acc.detach().clamp(lo, hi))
    zs = z + adt * zi
    return a, torch.where((zs > lo) & (zs < hi), zs, zs.detach().clamp(lo, hi))


@pytest.mark.parametrize("solver", ["euler", "tsit5"])
@pytest.mark.parametrize("env_name,deadtime", hf.CASES)
def test_gradients_equal_the_chain_of_differentiable_steps(env_name, deadtime, solver):
    """Each side holds 1e-8 to the twin (test 1 here, tests/test_gpu_step_vjp.py there): 2e-8 between them."""
    B, K = hf.B_MAIN, 5
    spec = case_spec(env_name, deadtime)
    inp = hf.feedback_inputs(env_name, spec, B, K)
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    run = forward(env, inp, K, 1, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    group = hv.cotangent_groups(np.random.default_rng(6), B, K + 1, OW, S, K, A)[0]
    got = explicit(run, group)
    # the parent's route: K differentiable vmap_step calls, the policy in torch
    env.differentiable = True
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    gain, igain, ff, z0 = leaf(run["gain"]), leaf(run["igain"]), leaf(run["ff"]), leaf(run["z0"])
    st0 = [leaf(getattr(run["state"].physical_state, n)) for n in env.STATE_FIELDS]
    s = env.State(env.PhysicalState(*st0), run["state"].PRNGKey, run["state"].additions, run["state"].reference)
    # row 0's observation with a graph: the twin's observe in torch on the device (the package's own is a kernel without one)
    ob = hv.Twin(env_name, spec, solver, "step").observe(st0)
    print(f"{env_name}: observation row 0, torch against the kernel's: {float((ob.detach() - run['obs'][:, 0]).abs().max()):.3e}")
    d = lambda v: _dev(v, env)
    loss = (ob * d(group["obs"][:, 0])).sum() + sum((l * d(g[:, 0])).sum() for l, g in zip(st0, group["states"]))
    z, acts = z0, []
    for k in range(K):
        a, z = _torch_policy(ob, gain, igain, ff[:, k], z, hf.CLIP[0], hf.CLIP[1], spec["tau"])
        acts.append(a)
        ob, s = env.vmap_step(s, a)
        loss = loss + (ob * d(group["obs"][:, k + 1])).sum() + (a * d(group["actions"][:, k])).sum()
        loss = loss + sum((getattr(s.physical_state, n) * d(g[:, k + 1])).sum() for n, g in zip(env.STATE_FIELDS, group["states"]))
    loss = loss + (z * d(group["z"])).sum() + sum((getattr(s.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["last"]))
    gr = torch.autograd.grad(loss, st0 + [gain, igain, ff, z0])
    torch.cuda.synchronize()
    env.differentiable = False
    chain_actions = torch.stack(acts, dim=1).detach()
    da = float((chain_actions - run["actions"]).abs().max())
    print(f"{env_name} dead={deadtime} {solver}: forward actions bit-equal {torch.equal(chain_actions, run['actions'])}, distance {da:.3e}; "
          f"last observation row bit-equal {torch.equal(ob.detach(), run['obs'][:, -1])}")
    want = dict(state0=[_np(g) for g in gr[:S]], gain=_np(gr[S]), igain=_np(gr[S + 1]), ff=_np(gr[S + 2]), z0=_np(gr[S + 3]))
    check(compare(got, want), 2e-8, f"{env_name} dead={deadtime} {solver} vs the chain of steps")


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("solver", hf.SOLVERS)
@pytest.mark.parametrize("env_name,deadtime", hf.CASES)
def test_fp32_gradients_within_32_forward_floors(env_name, deadtime, solver):
    """The floor: helpers_vjp.obs_floor of the fp32 closed-loop forward (code this feature does not touch) against the twin on the
    same fp32-representable inputs, over the kept environments."""
    spec, inp64 = hf.main_case(env_name, deadtime)
    inp = rounded(inp64, torch.float32)
    K, sub = hf.K_MAIN, hf.substeps_of(env_name)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, K, sub)
    keep = twin.kink_distance().numpy() >= KINK_MARGIN
    excluded = 1.0 - float(np.mean(keep))
    env, _, _, _ = make_env(env_name, hf.B_MAIN, torch.float32, solver, spec=spec)
    run = forward(env, inp, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    floor = obs_floor(_np(run["obs"]), out["obs"].detach().numpy(), env_name, keep)
    groups = hv.cotangent_groups(np.random.default_rng(5), hf.B_MAIN, K * sub + 1, OW, S, K, A)[:1]
    groups = [{k: (None if v is None else ([x.astype(np.float32).astype(np.float64) for x in v] if isinstance(v, list)
                                            else v.astype(np.float32).astype(np.float64))) for k, v in groups[0].items()}]
    want = hv.twin_grads(lv, out, groups, OW)[0]
    got = explicit(run, groups[0])
    print(f"{env_name} dead={deadtime} {solver}: excluded {excluded:.4f}, forward floor {floor:.3e}")
    assert excluded <= KINK_CAP
    check(compare(got, want, keep), 32 * floor, f"{env_name} dead={deadtime} {solver} fp32")


# ---------------------------------------------------------------------------------------------------------------- 4, 9
def _raw_call(env, run, alloc, group, want_gain=True, gain_batch=None):
    """excenv_sim_feedback_vjp straight through ctypes on buffers from `alloc` (helpers_guard.Plain / Carved) -> (outputs, workspace
    tensor, layout of the workspace). The forward's tensors are copied into the provider's buffers."""
    B, S, A, OW = env.batch_size, env.physical_state_dim, env.action_dim, env._obs_dim()
    K, sub, dt = run["K"], run["sub"], env.dtype
    rows = K * sub + 1
    npdt = NP_DTYPE[dt]
    lane = lambda t, perm: np.ascontiguousarray(t.detach().cpu().numpy().transpose(*perm)).astype(npdt)
    integral = run["igain"] is not None
    gb = run["gain"].shape[0] if run["gain"].ndim == 3 else 1
    glay = lambda g: lane(g, (1, 2, 0)) if g.ndim == 3 else g.detach().cpu().numpy().astype(npdt)[:, :, None]
    alloc("gain", (A, OW, gb), dt, "gains", fill=glay(run["gain"]))
    if integral:
        alloc("integral_gain", (A, OW, gb), dt, "gains", fill=glay(run["igain"]))
        if run["z0"] is not None:
            alloc("z_in", (A, B), dt, "z", fill=lane(run["z0"], (1, 0)))
    alloc("obs_traj", (rows, OW, B), dt, "obs", fill=lane(run["obs"], (1, 2, 0)))
    tn = [f"state_traj[{j}]" for j in range(S)]
    for n, f in zip(tn, env.STATE_FIELDS):
        alloc(n, (rows, B), dt, "straj", fill=lane(getattr(run["states"].physical_state, f), (1, 0)))
    alloc("actions", (K, A, B), dt, "actions", fill=lane(run["actions"], (1, 2, 0)))
    cot = lambda v, perm: np.ascontiguousarray(np.asarray(v).transpose(*perm)).astype(npdt)
    if group.get("obs") is not None:
        alloc("grad_obs", (rows, OW, B), dt, "cot", fill=cot(group["obs"], (1, 2, 0)))
    gsn = glast = None
    if group.get("states") is not None:
        gsn = [f"grad_states[{j}]" for j in range(S)]
        for n, g in zip(gsn, group["states"]):
            alloc(n, (rows, B), dt, "cot", fill=cot(g, (1, 0)))
    if group.get("last") is not None:
        glast = [f"grad_last_state[{j}]" for j in range(S)]
        for n, g in zip(glast, group["last"]):
            alloc(n, (B,), dt, "cot", fill=np.asarray(g).astype(npdt))
    if group.get("actions") is not None:
        alloc("grad_actions", (K, A, B), dt, "cot", fill=cot(group["actions"], (1, 2, 0)))
    if integral and group.get("z") is not None:
        alloc("grad_z", (A, B), dt, "cot", fill=cot(group["z"], (1, 0)))
    out = {}
    g0 = [f"grad_state0[{j}]" for j in range(S)]
    for n in g0:
        out[n] = alloc(n, (B,), dt, "out")
    out["grad_ff"] = alloc("grad_ff", (K, A, B), dt, "out")
    if integral:
        out["grad_zi"] = alloc("grad_zi", (K, A, B), dt, "out")
        out["grad_z0"] = alloc("grad_z0", (A, B), dt, "out")
    if want_gain:
        out["grad_gain"] = alloc("grad_gain", (A, OW, gb), dt, "out")
        if integral:
            out["grad_integral_gain"] = alloc("grad_integral_gain", (A, OW, gb), dt, "out")
    lib = _native.lib()
    nc = len(env.control_state)
    ws_bytes = lib.excenv_sim_feedback_vjp_workspace_bytes(env.ENV_ID, _native.dtype_id(dt), B, K, nc, gb, int(integral))
    ws = alloc("workspace", (max(ws_bytes, 1),), torch.uint8, "workspace", role="scratch")
    alloc.ready()
    have = lambda n: alloc.addr(n) if _has(alloc, n) else None
    arr = lambda names: None if names is None else (ctypes.c_void_p * len(names))(*[alloc.addr(n) for n in names])
    p_traj, p_gs, p_gl, p_g0 = arr(tn), arr(gsn), arr(glast), arr(g0)
    ad = lambda a: None if a is None else ctypes.addressof(a)
    lo, hi = (-np.inf, np.inf) if run["clip"] is None else run["clip"]
    rec = _native.FeedbackVjp(alloc.addr("gain"), have("integral_gain"), gb, lo, hi, alloc.addr("obs_traj"), ad(p_traj), alloc.addr("actions"),
                              have("z_in"), have("grad_obs"), ad(p_gs), ad(p_gl), have("grad_actions"), have("grad_z"), ad(p_g0),
                              alloc.addr("grad_ff"), have("grad_zi"), have("grad_z0"), have("grad_gain"), have("grad_integral_gain"))
    props, keep = env._props_for(env.env_properties, B)
    control, refs = env._control(run["state"], (B,))
    with _native._on_device(env.device):
        rc = lib.excenv_sim_feedback_vjp(env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, K, sub, ctypes.byref(props),
                                         _native._ref(control), float(run["tau"]), float(env.tau), ctypes.byref(rec),
                                         alloc.addr("workspace"), ws_bytes, None, _native._raw_stream(env.device))
    assert rc == 0, lib.excenv_last_error()
    assert _native.last_launch() == "sim_feedback_vjp_kernel"
    torch.cuda.synchronize()
    elem = 4 if dt == torch.float32 else 8
    up = lambda n: (n + 255) // 256 * 256
    layout = dict(z=(0, elem * K * A * B if integral else 0))
    z_end = up(layout["z"][1]) if integral else 0
    layout["terms"] = (z_end, z_end + (elem * (2 if integral else 1) * A * OW * B if gb == 1 else 0))
    return out, ws, layout


def _has(alloc, name):
    try:
        alloc.addr(name)
        return True
    except (KeyError, StopIteration):
        return False


@pytest.mark.parametrize("with_z0", [True, False], ids=["integrator_state", "zeros"])
@pytest.mark.parametrize("env_name,deadtime,sub", [("cartpole", None, 3), ("mass_spring_damper", None, 1), ("pmsm", 1, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_pre_pass_ends_on_the_forwards_integrator_state_bit_for_bit(env_name, deadtime, sub, with_z0, dtype):
    from helpers_guard import Plain

    spec = case_spec(env_name, deadtime)
    B, K = hf.B_MAIN, hf.K_MAIN
    inp = dict(hf.feedback_inputs(env_name, spec, B, K))
    if not with_z0:
        inp["z0"] = None
    env, _, _, _ = make_env(env_name, B, dtype, "rk4", spec=spec)
    run = forward(env, inp, K, sub, spec["tau"])
    alloc = Plain()
    _, ws, layout = _raw_call(env, run, alloc, dict(last=[np.ones(B)] * env.physical_state_dim))
    A = env.action_dim
    zrows = ws[layout["z"][0]:layout["z"][1]].view(dtype).view(K, A, B)
    same = torch.equal(zrows[K - 1].t(), run["z"])
    clamped = int((run["z"].abs() >= 1.0).sum())
    print(f"{env_name} substeps {sub} {dtype} z0={with_z0}: last pre-pass row == returned z: {same}; {clamped} entries on the clamp")
    assert same and bool(torch.isfinite(zrows).all())


GUARD_CASES = [("pendulum", None, torch.float32, "euler", False), ("pmsm", 1, torch.float64, "tsit5", True),
               ("acrobot", None, torch.float64, "rk4", False)]


@pytest.mark.parametrize("B", [hf.B_MAIN, 1])
@pytest.mark.parametrize("env_name,deadtime,dtype,solver,per_env", GUARD_CASES, ids=lambda v: str(v))
def test_guard_bands_the_launches_write_their_outputs_and_nothing_else(env_name, deadtime, dtype, solver, per_env, B):
    """helpers_guard.Arena: every buffer of the call carved from one pattern-filled allocation. Guards untouched, inputs unchanged,
    every output element written; of the workspace, the integrator rows and (one gain set for all) the per-environment terms are
    written completely — its alignment padding and the unused part of the batch sum's partials are not outputs."""
    from helpers_guard import Carved, Plain, arena_bytes

    spec = case_spec(env_name, deadtime)
    K, sub = hf.K_MAIN, hf.substeps_of(env_name)
    inp = hf.feedback_inputs(env_name, spec, B, K, per_env_gains=per_env)
    env, _, _, _ = make_env(env_name, B, dtype, solver, spec=spec)
    run = forward(env, inp, K, sub, spec["tau"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    group = hv.cotangent_groups(np.random.default_rng(9), B, K * sub + 1, OW, S, K, A)[0]
    plain = Plain()
    ref, _, _ = _raw_call(env, run, plain, group)
    elem = 4 if dtype == torch.float32 else 8
    for place in ({}, {"out": elem, "cot": elem}, {"workspace": 16, "gains": elem}):
        carved = Carved(arena_bytes(plain.sizes), place)
        got, ws, layout = _raw_call(env, run, carved, group)
        carved.arena.check()
        for name, (a, b) in layout.items():
            part = ws[a:b]
            if part.numel():
                words = part.view(torch.int32 if elem == 4 else torch.int64)
                assert int((words == -1).sum()) == 0, f"workspace part {name!r} not written completely"
        bad = [n for n in ref if not torch.equal(ref[n], got[n])]
        print(f"guard {env_name} {dtype} {solver} B={B} per-env gains={per_env} @ {place or 'offset 0'}: differ from the plain run: {bad}")
        assert not bad


# ---------------------------------------------------------------------------------------------------------------- 5
def _form(env_name, deadtime, solver, B, K, dtype=torch.float64, control=None, clip=hf.CLIP, seed=72, **kw):
    """One form: inputs, the twin's gradients and the explicit form's for the full cotangent group -> (got, want, run, inp)"""
    spec = case_spec(env_name, deadtime)
    sub = hf.substeps_of(env_name)
    inp = hf.feedback_inputs(env_name, spec, B, K, seed=seed, control=control, **kw)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, K, sub, clip=clip, control=control)
    env, _, _, _ = make_env(env_name, B, dtype, solver, spec=spec, control_state=list(control) if control else None)
    run = forward(env, inp, K, sub, spec["tau"], clip=clip, control=control)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    group = hv.cotangent_groups(np.random.default_rng(11), B, K * sub + 1, OW, S, K, A, integral=inp["igain"] is not None)[0]
    want = hv.twin_grads(lv, out, [group], OW)[0]
    return explicit(run, group), want, run, inp, group


FORM_CASES = [("cartpole", None, "rk4"), ("pmsm", 1, "euler")]


@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_broadcast_gains_are_the_batch_sum_of_the_per_environment_result(env_name, deadtime, solver):
    got, want, run, inp, group = _form(env_name, deadtime, solver, hf.B_MAIN, hf.K_MAIN, per_env_gains=False)
    check(compare(got, want, per_env=False), TOL, f"{env_name} broadcast gains")
    env = run["env"]
    B, A, OW = env.batch_size, env.action_dim, env._obs_dim()
    assert tuple(got["gain"].shape) == (A, OW) and tuple(got["igain"].shape) == (A, OW)
    assert_batch_sum_identity(run, group, got, env_name)


def assert_batch_sum_identity(run, group, got, label):
    """One gain set for all: its gradients equal, bit for bit, excenv_param_grad_sum of the per-environment gradients of the same
    gains, one copy per environment, and every other gradient is the per-environment launch's -> that launch's result"""
    env = run["env"]
    B, A, OW = env.batch_size, env.action_dim, env._obs_dim()
    # the same gains, one copy per environment: per-environment gradients, summed by excenv_param_grad_sum
    rep = dict(run)
    rep["gain"] = run["gain"][None].expand(B, A, OW).contiguous()
    rep["igain"] = None if run["igain"] is None else run["igain"][None].expand(B, A, OW).contiguous()
    per = explicit(rep, group)
    for name, j in (("gain", 1), ("igain", 2)):
        if per["raw"][j] is None:
            assert got["raw"][j] is None
            continue
        t = per["raw"][j]  # [B, A, OW] over lane-major memory
        leaves = [t[:, q, o] for q in range(A) for o in range(OW)]
        assert all(l.is_contiguous() for l in leaves)
        sums = []
        for c in range(0, len(leaves), _native.MAX_STATIC):
            sums += env._param_grad_sum(leaves[c:c + _native.MAX_STATIC])
        summed = torch.stack(sums).reshape(A, OW)
        same = torch.equal(summed, got["raw"][j])
        print(f"{label} {name}: broadcast result == excenv_param_grad_sum of the per-environment result: {same}")
        assert same
    for a, b in zip(per["state0"], got["state0"]):
        assert np.array_equal(a, b)
    assert np.array_equal(per["ff"], got["ff"])
    assert (per["z0"] is None and got["z0"] is None) or np.array_equal(per["z0"], got["z0"])
    return per


def test_mixed_pair_broadcast_gain_with_per_environment_integral_gain():
    env_name, solver, B, K = "mass_spring_damper", "tsit5", hf.B_MAIN, hf.K_MAIN
    spec = case_spec(env_name, None)
    sub = hf.substeps_of(env_name)
    inp = dict(hf.feedback_inputs(env_name, spec, B, K))
    inp["gain"] = inp["gain"][0]  # [A, OW] next to a [B, A, OW] integral gain
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, K, sub)
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    run = forward(env, inp, K, sub, spec["tau"])
    group = hv.cotangent_groups(np.random.default_rng(12), B, K * sub + 1, 2, 2, K, 1)[0]
    got = explicit(run, group)
    assert tuple(got["gain"].shape) == (1, 2) and tuple(got["igain"].shape) == (B, 1, 2)
    check(compare(got, hv.twin_grads(lv, out, [group], 2)[0], per_env=False), TOL, "mixed pair")


@pytest.mark.parametrize("env_name,deadtime,control", [("cartpole", None, ("velocity", "theta")), ("pmsm", 0, ("i_d", "i_q"))])
def test_two_control_columns_their_gains_get_gradients(env_name, deadtime, control):
    got, want, run, inp, _ = _form(env_name, deadtime, "rk4", hf.B_MAIN, hf.K_MAIN, control=control)
    check(compare(got, want), TOL, f"{env_name} control {control}")
    O = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][2]
    ref_cols = float(np.abs(got["gain"][:, :, O:]).max())
    print(f"{env_name}: largest gain gradient on a reference column {ref_cols:.3e}")
    assert got["gain"].shape[2] == O + 2 and ref_cols > 0


@pytest.mark.parametrize("what", ["no_feedforward", "no_integral", "no_clip"])
@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_without_feedforward_integrator_or_clamp(env_name, deadtime, solver, what):
    kw = dict(feedforward=what != "no_feedforward", integral=what != "no_integral")
    got, want, run, inp, _ = _form(env_name, deadtime, solver, hf.B_MAIN, hf.K_MAIN, clip=None if what == "no_clip" else hf.CLIP, **kw)
    assert (got["igain"] is None) == (what == "no_integral") and (got["z0"] is None) == (what == "no_integral")
    if what == "no_feedforward":  # the gradient with respect to the pre-clamp action is returned all the same
        assert want["ff"] is None and got["ff"] is not None
        got = dict(got, ff=None)
    check(compare(got, want), TOL, f"{env_name} {what}")


@pytest.mark.parametrize("B,K", [(hf.B_MAIN, 1), (1, hf.K_MAIN), (hf.B_MAIN, 0), (1, 0)])
@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_single_rows_single_environments_and_no_rows(env_name, deadtime, solver, B, K):
    got, want, run, inp, _ = _form(env_name, deadtime, solver, B, K, seed=72 + 10 * B + K)
    assert got["ff"].shape == (B, K, run["env"].action_dim)
    check(compare(got, want), TOL, f"{env_name} B={B} K={K}")


def test_per_environment_gains_pmsm_fp64_tsit5():
    """The tightest register case (256 of 256): per-environment gains, a private run of LDS per lane"""
    for deadtime in (0, 1):
        got, want, _, _, _ = _form("pmsm", deadtime, "tsit5", 2 * 256 + 70, 3, seed=31)
        check(compare(got, want), TOL, f"pmsm dead={deadtime} tsit5 per-environment gains")


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("env_name,deadtime,solver", [("pendulum", None, "tsit5"), ("acrobot", None, "rk4"), ("pmsm", 1, "euler"),
                                                     ("fluid_tank", None, "rk4")])
def test_zero_gains_are_the_open_loop_reverse_kernel(env_name, deadtime, solver):
    spec = case_spec(env_name, deadtime)
    B, K, sub = hf.B_MAIN, hf.K_MAIN, hf.substeps_of(env_name)
    inp = dict(hf.feedback_inputs(env_name, spec, B, K, integral=False))
    inp["gain"] = np.zeros_like(inp["gain"])
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    run = forward(env, inp, K, sub, spec["tau"], clip=None)
    assert torch.equal(run["actions"], run["ff"])
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    group = hv.cotangent_groups(np.random.default_rng(13), B, K * sub + 1, OW, S, K, A, integral=False)[0]
    group = dict(group, actions=None)
    got = explicit(run, group)
    keep = env.sim_ahead_semantics, env.launch_opts
    env.sim_ahead_semantics, env.launch_opts = "step", _native.launch_opts(envs_per_lane=1)
    try:
        ga, gs = env.vmap_sim_ahead_vjp(run["states"], run["actions"], spec["tau"], spec["tau"] * sub, _dev(group["obs"], env),
                                        [_dev(g, env) for g in group["states"]], [_dev(g, env) for g in group["last"]])
        assert env.last_vjp_launch == "sim_ahead_vjp_kernel (V=1)"
    finally:
        env.sim_ahead_semantics, env.launch_opts = keep
    torch.cuda.synchronize()
    want = dict(state0=[_np(getattr(gs, n)) for n in env.STATE_FIELDS], gain=None, igain=None, ff=_np(ga), z0=None)
    bits = torch.equal(ga, got["raw"][3]) and all(torch.equal(getattr(gs, n), getattr(got["raw"][0], n)) for n in env.STATE_FIELDS)
    print(f"{env_name} {solver}: zero gains bit-equal to vmap_sim_ahead_vjp: {bits}")
    check(compare(dict(got, gain=None), want), TOL, f"{env_name} {solver} zero gains")
    assert float(np.abs(got["gain"]).max()) > 0  # the gains' own gradient is not zero at zero gains


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("env_name,deadtime,solver", FORM_CASES)
def test_recording_form_fills_the_grads_with_the_explicit_forms_bits(env_name, deadtime, solver):
    spec = case_spec(env_name, deadtime)
    B, K, sub = hf.B_MAIN, hf.K_MAIN, hf.substeps_of(env_name)
    inp = hf.feedback_inputs(env_name, spec, B, K)
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    plain = forward(env, inp, K, sub, spec["tau"], differentiable=True)  # no input requires grad: the plain path
    assert plain["obs"].grad_fn is None and plain["actions"].grad_fn is None and env.last_feedback_vjp_launch == ""
    group = hv.cotangent_groups(np.random.default_rng(14), B, K * sub + 1, OW, S, K, A)[0]
    want = explicit(plain, group)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    gain, igain, ff, z0 = leaf(plain["gain"]), leaf(plain["igain"]), leaf(plain["ff"]), leaf(plain["z0"])
    st0 = [leaf(getattr(plain["state"].physical_state, n)) for n in env.STATE_FIELDS]
    s = env.State(env.PhysicalState(*st0), plain["state"].PRNGKey, plain["state"].additions, plain["state"].reference)
    obs, states, last, actions, z = env.vmap_sim_ahead_feedback(s, gain, K, spec["tau"], spec["tau"] * sub, feedforward=ff, integral_gain=igain,
                                                                integrator_state=z0, differentiable=True)
    assert all(t.grad_fn is not None for t in (obs, actions, z)) and torch.equal(obs, plain["obs"]) and torch.equal(z, plain["z"])
    d = lambda v: _dev(v, env)
    loss = (obs * d(group["obs"])).sum() + (actions * d(group["actions"])).sum() + (z * d(group["z"])).sum()
    loss = loss + sum((getattr(states.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["states"]))
    loss = loss + sum((getattr(last.physical_state, n) * d(g)).sum() for n, g in zip(env.STATE_FIELDS, group["last"]))
    loss.backward()
    torch.cuda.synchronize()
    assert env.last_feedback_vjp_launch == "sim_feedback_vjp_kernel"
    gs, gg, ggi, gff, gz0 = want["raw"]
    pairs = [("gain", gain.grad, gg), ("integral_gain", igain.grad, ggi), ("feedforward", ff.grad, gff), ("integrator_state", z0.grad, gz0)]
    pairs += [(n, l.grad, getattr(gs, n)) for n, l in zip(env.STATE_FIELDS, st0)]
    for name, a, b in pairs:
        print(f"{env_name} {name}: .grad == explicit form: {torch.equal(a, b)}")
        assert torch.equal(a, b), name


@pytest.mark.parametrize("env_name,deadtime,control", [("cartpole", None, ("velocity", "theta")), ("pmsm", 1, ("i_d", "i_q"))])
def test_a_reward_loss_reaches_the_gains(env_name, deadtime, control):
    from helpers_step_vjp import reward64

    solver = "rk4"
    spec = case_spec(env_name, deadtime)
    B, K, sub = hf.B_MAIN, hf.K_MAIN, hf.substeps_of(env_name)
    inp = hf.feedback_inputs(env_name, spec, B, K, control=control)
    twin, lv, out = hv.twin_run(env_name, spec, solver, inp, K, sub, control=control)
    rows = K * sub + 1
    rew = sum(reward64(env_name, spec, control, [s[:, n] for s in out["states"]], inp["refs"]) for n in range(1, rows))
    wrt = [lv["gain"], lv["igain"], lv["ff"], lv["z0"]] + lv["st"]
    gr = torch.autograd.grad(-rew.sum(), wrt, allow_unused=True)
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec, control_state=list(control))
    env.differentiable = True
    plain = forward(env, inp, K, sub, spec["tau"], control=control)
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    gain, igain, ff, z0 = leaf(plain["gain"]), leaf(plain["igain"]), leaf(plain["ff"]), leaf(plain["z0"])
    st0 = [leaf(getattr(plain["state"].physical_state, n)) for n in env.STATE_FIELDS]
    s = env.State(env.PhysicalState(*st0), plain["state"].PRNGKey, plain["state"].additions, plain["state"].reference)
    obs, states, last, actions, z = env.vmap_sim_ahead_feedback(s, gain, K, spec["tau"], spec["tau"] * sub, feedforward=ff, integral_gain=igain,
                                                                integrator_state=z0, differentiable=True)
    reward, _, _ = env.vmap_generate_rew_trunc_term_ahead(states, actions)
    (-reward.sum()).backward()
    torch.cuda.synchronize()
    got = dict(state0=[_np(l.grad) if l.grad is not None else np.zeros(B) for l in st0], gain=_np(gain.grad), igain=_np(igain.grad),
               ff=_np(ff.grad), z0=_np(z0.grad))
    z_ = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy()
    want = dict(gain=z_(gr[0], lv["gain"]), igain=z_(gr[1], lv["igain"]), ff=z_(gr[2], lv["ff"]), z0=z_(gr[3], lv["z0"]),
                state0=[z_(g, l) for g, l in zip(gr[4:], lv["st"])])
    assert env.last_feedback_vjp_cotangents["obs"] is False and any(env.last_feedback_vjp_cotangents["states"])
    check(compare(got, want), TOL, f"{env_name} reward loss through the closed loop")


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("env_name,deadtime", [("mass_spring_damper", None), ("pmsm", 0)])
def test_directional_finite_difference_in_the_gains(env_name, deadtime):
    """<grad_gain, d_gain> + <grad_integral_gain, d_igain> per environment against (L(+h) - L(-h)) / 2h of three forward launches; h and
    the bound are those of tests/test_gpu_reward_vjp.py's directional test (1e-5, 1e-6 of the largest derivative). Environments
    inside KINK_MARGIN of a kink or clamp bound are excluded: a difference quotient across a kink is not a derivative."""
    solver, h = "rk4", 1e-5
    spec = case_spec(env_name, deadtime)
    B, K, sub = hf.B_MAIN, hf.K_MAIN, hf.substeps_of(env_name)
    inp = hf.feedback_inputs(env_name, spec, B, K)
    twin, _, _ = hv.twin_run(env_name, spec, solver, inp, K, sub)
    keep = twin.kink_distance().numpy() >= KINK_MARGIN
    rng = np.random.default_rng(15)
    dg, dgi = rng.normal(size=inp["gain"].shape), rng.normal(size=inp["igain"].shape) * float(np.abs(inp["igain"]).max())
    env, _, _, _ = make_env(env_name, B, torch.float64, solver, spec=spec)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    w = rng.normal(size=(B, K * sub + 1, OW))

    def loss_rows(sign):
        moved = dict(inp, gain=inp["gain"] + sign * h * dg, igain=inp["igain"] + sign * h * dgi)
        return _np(forward(env, moved, K, sub, spec["tau"])["obs"])

    run = forward(env, inp, K, sub, spec["tau"])
    got = explicit(run, dict(obs=w))
    dd = (got["gain"] * dg).sum(axis=(1, 2)) + (got["igain"] * dgi).sum(axis=(1, 2))
    fd = (w * (loss_rows(+1) - loss_rows(-1))).sum(axis=(1, 2)) / (2 * h)
    scale = float(np.max(np.abs(fd[keep])))
    err = float(np.max(np.abs(dd - fd)[keep])) / scale
    print(f"{env_name} dead={deadtime}: directional derivative rel err {err:.3e} (scale {scale:.3e}), excluded {1 - float(np.mean(keep)):.4f}")
    assert 1 - float(np.mean(keep)) <= KINK_CAP
    assert err <= 1e-6
