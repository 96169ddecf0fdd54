#!/usr/bin/env python3
"""What a differentiable closed-loop step costs, in one process: PMSM (i_d, i_q) and pendulum (theta), Euler fp32.
At B = 2^15, per-step wall time (host clock around forward + backward of `--inner` steps, ending in a device synchronise; median of
`--reps` such windows) of
  step_route        vmap_gym_step under env.differentiable, then backward of cotangents on obs, reward and the new state: two launches
  trajectory_route  the same step as a trajectory of one row: a K = 1 differentiable vmap_sim_ahead under "step", then
                    vmap_generate_rew_trunc_term_ahead, then backward (lane-major cotangents, the favourable case): four launches
At B = 2^20, the excenv_step_vjp launch alone (pre-built arguments, `--inner` launches between two device events) with all three
cotangent groups, its algorithmic bytes from excenv_step_vjp_bytes and the achieved fraction of the 8 TB/s HBM peak, next to
excenv_step (the forward of an environment without controlled fields, excenv_step_bytes) measured the same way.
usage: tools/step_vjp_cost.py [--small B] [--large B] [--reps N] [--inner N] [--json FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK = 8.0e12  # bytes / s
DEV = "cuda:0"


def make(reg, name, control, B):
    env = reg.make(batch_size=B, dtype=torch.float32, device=DEV, control_state=list(control))
    _, state = env.vmap_reset()
    if name == "pmsm":
        state.physical_state.omega_el = torch.rand(B, device=DEV) * 600
        state.physical_state.epsilon = (torch.rand(B, device=DEV) - 0.5) * 6
    for n in control:
        nz = getattr(env.env_properties.physical_normalizations, n)
        setattr(state.reference, n, (torch.rand(B, device=DEV) * 2 - 1) * float(nz.max))
    return env, state


def wall_us(fn, reps, inner, warm=3):
    """median over `reps` windows of the host time of one fn(), each window `inner` calls ending in a synchronise"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / inner * 1e6)
    return statistics.median(us)


def device_us(fn, reps, inner, warm=3):
    """median over `reps` windows of the device time of one fn(), `inner` calls between two events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        us.append(float(t0.elapsed_time(t1)) / inner * 1e3)
    return statistics.median(us)


def routes(name, reg, control, B, reps, inner):
    env, state = make(reg, name, control, B)
    S, A = env.physical_state_dim, env.action_dim
    action = (torch.rand(B, A, device=DEV) - 0.5) * 1.5
    env.differentiable = True
    obs, rew, _, _, s1 = env.vmap_gym_step(state, action.clone().requires_grad_(True))
    g_obs, g_rew = torch.randn_like(obs), torch.randn_like(rew)
    g_leaves = [torch.randn(B, device=DEV) for _ in range(S)]

    def step_route():
        a = action.detach().requires_grad_(True)
        o, r, _, _, s = env.vmap_gym_step(state, a)
        torch.autograd.backward([o, r] + [getattr(s.physical_state, n) for n in env.STATE_FIELDS], [g_obs, g_rew] + g_leaves)
        return a.grad

    env_p, state_p = make(reg, name, control, B)
    for n in env.STATE_FIELDS:  # the same inputs
        setattr(state_p.physical_state, n, getattr(state.physical_state, n))
        setattr(state_p.reference, n, getattr(state.reference, n))
    env_p.sim_ahead_semantics = "step"
    env_p.differentiable = True
    actions = env_p.new_actions_buffer(1)
    actions.copy_(action[:, None, :])
    tau = env_p.tau
    o2, st2, _ = env_p.vmap_sim_ahead(state_p, actions.detach().requires_grad_(True), tau, tau)
    r2, _, _ = env_p.vmap_generate_rew_trunc_term_ahead(st2, actions)
    g_obs2 = torch.empty_like(o2.detach()).zero_()  # empty_like keeps the lane-major strides
    g_obs2[:, 1] = g_obs
    g_rew2 = torch.empty_like(r2.detach()).copy_(g_rew[:, None, :])

    def trajectory_route():
        a = actions.detach().requires_grad_(True)
        o, st, last = env_p.vmap_sim_ahead(state_p, a, tau, tau)
        r, _, _ = env_p.vmap_generate_rew_trunc_term_ahead(st, a)
        torch.autograd.backward([o, r] + [getattr(last.physical_state, n) for n in env.STATE_FIELDS], [g_obs2, g_rew2] + g_leaves)
        return a.grad

    ga, gb = step_route(), trajectory_route()
    torch.cuda.synchronize()
    diff = float((ga - gb[:, 0]).abs().max() / gb.abs().max())
    a_us, b_us = wall_us(step_route, reps, inner), wall_us(trajectory_route, reps, inner)
    a_us2, b_us2 = wall_us(step_route, reps, inner), wall_us(trajectory_route, reps, inner)  # alternated once more: the spread
    return {"workload": f"{name} {'+'.join(control)} euler fp32", "B": B, "step_route_us": [round(a_us, 2), round(a_us2, 2)],
            "trajectory_route_us": [round(b_us, 2), round(b_us2, 2)], "grad_action_rel_diff": diff,
            "step_over_trajectory": round(min(a_us, a_us2) / min(b_us, b_us2), 3)}


def launch_alone(name, reg, control, B, reps, inner):
    from exciting_environments_amd import _native

    env, state = make(reg, name, control, B)
    S, A = env.physical_state_dim, env.action_dim
    action = (torch.rand(B, A, device=DEV) - 0.5) * 1.5
    obs, rew, _, _, s1 = env.vmap_gym_step(state, action)
    g_obs, g_rew = torch.randn_like(obs), torch.randn(B, device=DEV)
    g_leaves = [torch.randn(B, device=DEV) for _ in range(S)]
    st_in = [getattr(state.physical_state, n) for n in env.STATE_FIELDS]
    st_out = [getattr(s1.physical_state, n) for n in env.STATE_FIELDS]
    refs = [getattr(state.reference, n) for n in control]
    props, _keep = env._props_for(env.env_properties, B)
    ctl = _native.make_control([env.STATE_FIELDS.index(n) for n in control], refs)
    gs = [torch.empty(B, device=DEV) for _ in range(S)]
    ga = torch.empty(B, A, device=DEV)
    lib, stream = _native.lib(), _native.raw_stream(0)
    args = (env.ENV_ID, env._solver.id, _native.F32, B, ctypes.byref(props), ctypes.byref(ctl), float(env.tau), _native._ptrs(st_in),
            action.data_ptr(), _native._ptrs(st_out), g_obs.data_ptr(), _native._ptrs(g_leaves), g_rew.data_ptr(), _native._ptrs(gs),
            ga.data_ptr(), None, stream)

    def vjp():
        rc = lib.excenv_step_vjp(*args)
        assert rc == 0, lib.excenv_last_error()

    nbytes = _native.step_vjp_bytes(env.ENV_ID, env.dtype, len(control), True, True, True)
    us = device_us(vjp, reps, inner)
    out = {"workload": f"{name} {'+'.join(control)} euler fp32", "B": B,
           "step_vjp": {"launch": _native.last_launch(), "us": round(us, 2), "bytes_per_env": nbytes,
                        "fraction_of_peak": round(nbytes * B / (us * 1e-6) / PEAK, 4)}}
    # the forward of an environment without controlled fields: excenv_step's own fast path
    env0, state0 = make(reg, name, (), B)
    st0 = [getattr(state0.physical_state, n) for n in env0.STATE_FIELDS]
    props0, _keep0 = env0._props_for(env0.env_properties, B)
    out0 = [torch.empty(B, device=DEV) for _ in range(S)]
    obs0 = torch.empty(B, env0._obs_dim(), device=DEV)
    fargs = (env0.ENV_ID, env0._solver.id, _native.F32, B, ctypes.byref(props0), None, float(env0.tau), _native._ptrs(st0),
             action.data_ptr(), _native._ptrs(out0), obs0.data_ptr(), None, stream)

    def fwd():
        rc = lib.excenv_step(*fargs)
        assert rc == 0, lib.excenv_last_error()

    fbytes = _native.step_bytes(env0.ENV_ID, env0.dtype)
    fus = device_us(fwd, reps, inner)
    out["step"] = {"us": round(fus, 2), "bytes_per_env": fbytes, "fraction_of_peak": round(fbytes * B / (fus * 1e-6) / PEAK, 4)}
    out["step_vjp"]["of_step_bandwidth"] = round(out["step_vjp"]["fraction_of_peak"] / out["step"]["fraction_of_peak"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=1 << 15)
    ap.add_argument("--large", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "step_vjp_cost.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: no device, no figures"
    from exciting_environments_amd import EnvironmentRegistry

    res = {"routes": [], "launch": []}
    for name, reg, control in (("pmsm", EnvironmentRegistry.PMSM, ("i_d", "i_q")), ("pendulum", EnvironmentRegistry.PENDULUM, ("theta",))):
        r = routes(name, reg, control, a.small, a.reps, a.inner)
        print(json.dumps(r))
        res["routes"].append(r)
        r = launch_alone(name, reg, control, a.large, a.reps, a.inner)
        print(json.dumps(r))
        res["launch"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
