"""Guard bands around every buffer of excenv_sim_policy_vjp (helpers_guard): the C entry straight through ctypes, every buffer of the
call carved from one pattern-filled allocation. For every model, B = 1 and 326, K = 0, 1 and 7, the networks N2 / N1 / N0 and every
optional input present and absent: the guards are untouched, every input is unchanged (the parameter array included), every output
element is written, and the outputs equal those of the same call on ordinary tensors bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import exciting_environments_amd as excenvs
import helpers_policy as hp
import helpers_policy_vjp as hv
from exciting_environments_amd import _native
from helpers import NP_DTYPE, make_env, to_state
from helpers_guard import Carved, Plain, arena_bytes
from helpers_vjp import case_spec

pytestmark = pytest.mark.gpu

# which optional inputs a call has: the cotangent groups and the episode mask
VARIANTS = [("all", ("obs", "states", "last", "actions")), ("none", ()), ("obs", ("obs",)), ("states", ("states",)), ("last", ("last",)),
            ("actions", ("actions",)), ("all+reset", ("obs", "states", "last", "actions", "reset"))]
NETS = ("N2", "N1", "N0")


def _forward(env, inp, K, sub, tau):
    state = to_state(env, inp["st"])
    policy = excenvs.MLPPolicy(inp["W"], inp["b"], "tanh", device=env.device, dtype=env.dtype)
    nz = torch.as_tensor(inp["noise"][:, :K], dtype=env.dtype, device=env.device) if K > 0 else None
    obs, states, last, actions = env.vmap_sim_ahead_policy(state, policy, K, tau, tau * sub, noise=nz)
    torch.cuda.synchronize()
    return dict(policy=policy, obs=obs, states=states, actions=actions)


def _raw_call(env, run, alloc, K, sub, tau, group, reset):
    """excenv_sim_policy_vjp on buffers from `alloc` (helpers_guard.Plain / Carved) -> its outputs. The forward's tensors are
    copied into the provider's buffers."""
    B, S, A, OW = env.batch_size, env.physical_state_dim, env.action_dim, env._obs_dim()
    dt = env.dtype
    rows = K * sub + 1
    npdt = NP_DTYPE[dt]
    lane = lambda t, perm: np.ascontiguousarray(t.detach().cpu().numpy().transpose(*perm)).astype(npdt)
    cot = lambda v, perm: np.ascontiguousarray(np.asarray(v).transpose(*perm)).astype(npdt)
    policy = run["policy"]
    alloc("params", (policy.params.numel(),), dt, "params", fill=policy.params.detach().cpu().numpy())
    alloc("obs_traj", (rows, OW, B), dt, "obs", fill=lane(run["obs"], (1, 2, 0)))
    tn = [f"state_traj[{j}]" for j in range(S)]
    for n, f in zip(tn, env.STATE_FIELDS):
        alloc(n, (rows, B), dt, "straj", fill=lane(getattr(run["states"].physical_state, f), (1, 0)))
    if K > 0:
        alloc("actions", (K, A, B), dt, "actions", fill=lane(run["actions"], (1, 2, 0)))
    if reset is not None and K > 0:
        alloc("reset", (K, B), torch.uint8, "reset", fill=np.ascontiguousarray(reset.T).astype(np.uint8))
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
    if group.get("actions") is not None and K > 0:
        alloc("grad_actions", (K, A, B), dt, "cot", fill=cot(group["actions"], (1, 2, 0)))
    out = {}
    g0 = [f"grad_state0[{j}]" for j in range(S)]
    for n in g0:
        out[n] = alloc(n, (B,), dt, "out")
    if K > 0:
        out["grad_raw"] = alloc("grad_raw", (K, A, B), dt, "out")
    alloc.ready()
    have = lambda n: alloc.addr(n) if _has(alloc, n) else None
    arr = lambda ns: None if ns is None else (ctypes.c_void_p * len(ns))(*[alloc.addr(n) for n in ns])
    p_traj, p_gs, p_gl, p_g0 = arr(tn), arr(gsn), arr(glast), arr(g0)
    ad = lambda a: None if a is None else ctypes.addressof(a)
    widths = (ctypes.c_int32 * (_native.POLICY_MAX_LAYERS + 1))(*policy.widths)
    pol = _native.Policy(alloc.addr("params"), policy.n_layers, _native.ACT_TANH, widths, None, hp.CLIP[0], hp.CLIP[1])
    rec = _native.PolicyVjp(pol, alloc.addr("obs_traj"), ad(p_traj), have("actions"), have("reset"), have("grad_obs"), ad(p_gs), ad(p_gl),
                            have("grad_actions"), ad(p_g0), have("grad_raw"))
    props, keep = env._props_for(env.env_properties, B)
    lib = _native.lib()
    with _native._on_device(env.device):
        rc = lib.excenv_sim_policy_vjp(env.ENV_ID, env._solver.id, _native.dtype_id(dt), B, K, sub, ctypes.byref(props), None, float(tau),
                                       float(env.tau), ctypes.byref(rec), None, _native._raw_stream(env.device))
    assert rc == 0, lib.excenv_last_error()
    assert _native.last_launch() == "sim_policy_vjp_kernel"
    torch.cuda.synchronize()
    return out


def _has(alloc, name):
    try:
        alloc.addr(name)
        return True
    except (KeyError, StopIteration):
        return False


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("B", [hp.B_MAIN, 1])
@pytest.mark.parametrize("env_name,deadtime", hp.CASES[:5] + [("pmsm", 1)])
def test_the_launch_writes_its_outputs_and_nothing_else(env_name, deadtime, B, dtype):
    spec = case_spec(env_name, deadtime)
    solver = {"pendulum": "tsit5", "acrobot": "rk4", "pmsm": "tsit5"}.get(env_name, "euler")
    env, _, _, _ = make_env(env_name, B, dtype, solver, spec=spec)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    elem = 4 if dtype == torch.float32 else 8
    rng = np.random.default_rng(9)
    n = 0
    for K in (0, 1, hp.K_MAIN):
        runs = {}
        for v, (label, present) in enumerate(VARIANTS):
            net = NETS[(v + K) % 3]
            sub = 1 if "reset" in present else hp.substeps_of(env_name)
            if (net, sub) not in runs:
                inp = hp.policy_inputs(env_name, spec, hp.NETS[net], B, K)
                runs[net, sub] = _forward(env, inp, K, sub, spec["tau"])
            run = runs[net, sub]
            full = hv.cotangent_groups(rng, B, K * sub + 1, OW, S, K, A)[0]
            group = {k: g for k, g in full.items() if k in present}
            reset = (rng.random((B, K)) < 0.3) if "reset" in present else None
            plain = Plain()
            ref = _raw_call(env, run, plain, K, sub, spec["tau"], group, reset)
            place = ({}, {"out": elem, "cot": elem}, {"params": elem, "obs": 16, "reset": 1})[v % 3]
            carved = Carved(arena_bytes(plain.sizes), place)
            got = _raw_call(env, run, carved, K, sub, spec["tau"], group, reset)
            carved.arena.check()
            bad = [k for k in ref if not torch.equal(ref[k], got[k])]
            assert not bad, (env_name, B, K, net, label, bad)
            n += 1
    print(f"guard {env_name} {dtype} {solver} B={B}: {n} calls, guards untouched, inputs unchanged, outputs written")
