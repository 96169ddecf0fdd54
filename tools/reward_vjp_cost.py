#!/usr/bin/env python3
"""What a differentiable trajectory reward costs, over the same buffers in one process: PMSM (i_d, i_q) and pendulum (theta), Euler
fp32 at B = 2^20, K = 100 (options below). Per workload, median of the timed launches after warm-up:
  forward           the trajectory launch (vmap_sim_ahead into the outputs of a first call), w (A + O + n_control + S) per env-step
  rew_trunc_term    excenv_rew_trunc_term over the stored trajectory, w (S + n_refs + 1) + 1 + TW per element
  rew_vjp           excenv_rew_vjp, w (reads + n_refs + 1 + reads) per element (state rows, references, reward cotangent in; cotangent rows out)
  reverse_from_reward   the reverse trajectory launch fed by rew_vjp's state cotangents, w (2A + S + reads) per env-step
  reverse_from_obs      the reverse trajectory launch fed by a full observation cotangent, w (2A + S + O) per env-step — what a user
                        who rebuilds the reward from `observations` in torch pays before any of their torch passes
with algorithmic bytes and the achieved fraction of the 8 TB/s HBM peak, and the total "rew_vjp + reverse_from_reward" next to
"reverse_from_obs". The yardstick for rew_vjp is the forward's bandwidth of the same run.
usage: tools/reward_vjp_cost.py [--batch B] [--steps K] [--reps N] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK = 8.0e12  # bytes / s


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(float(t0.elapsed_time(t1)))
    return statistics.median(ms)


def workload(name, reg, control, B, K, reps):
    from exciting_environments_amd import _native

    env = reg.make(batch_size=B, dtype=torch.float32, device="cuda:0", control_state=list(control))
    _, state = env.vmap_reset()
    if name == "pmsm":
        state.physical_state.omega_el = torch.rand(B, device="cuda:0") * 600
        state.physical_state.epsilon = (torch.rand(B, device="cuda:0") - 0.5) * 6
    for n in control:
        nz = getattr(env.env_properties.physical_normalizations, n)
        setattr(state.reference, n, (torch.rand(B, device="cuda:0") * 2 - 1) * float(nz.max))
    actions = env.new_actions_buffer(K)
    actions.copy_((torch.rand(B, K, env.action_dim, device="cuda:0") - 0.5) * 1.5)
    tau = env.tau
    trip = env.vmap_sim_ahead(state, actions, tau, tau)
    obs, states, last = trip
    S, A, OW = env.physical_state_dim, env.action_dim, obs.shape[-1]
    nc = len(control)
    O = OW - nc
    rows = K + 1
    w = 4
    reads = sum(env._reward_reads())
    TW = _native.truncated_width(env.ENV_ID, nc)
    out = {"workload": f"{name} {'+'.join(control)} euler fp32", "B": B, "K": K, "reads": reads, "n_refs": nc}

    def rec(key, ms, bytes_per_step):
        total = bytes_per_step * B * K
        out[key] = {"ms": round(ms, 4), "bytes_per_env_step": bytes_per_step, "gbytes": round(total / 1e9, 3),
                    "fraction_of_peak": round(total / (ms * 1e-3) / PEAK, 4)}

    rec("forward", timed(lambda: env.vmap_sim_ahead(state, actions, tau, tau, out=trip), reps), w * (A + OW + S))
    # the two reward launches into fixed buffers (the Python methods allocate their outputs per call)
    leaves = [getattr(states.physical_state, n) for n in env.STATE_FIELDS]
    refs = env._rew_refs(states.reference, B, rows)
    ctl, ref_strides = env._rew_control(refs)
    props, keep = env._props_for(env.env_properties, B)
    rew = torch.empty((K, B), device="cuda:0")
    term = torch.empty((K, B), dtype=torch.bool, device="cuda:0")
    trunc = torch.empty((rows, B, TW), dtype=torch.bool, device="cuda:0")
    rec("rew_trunc_term", timed(lambda: _native.rew_trunc_term(env.ENV_ID, env.dtype, B, rows, props, ctl, ref_strides, leaves, 1, B, rew,
                                                               term, trunc, _native.LAYOUT_LANE_MAJOR), reps), w * (S + nc + 1) + 1 + TW)
    g = torch.empty((K, B), device="cuda:0").normal_()
    outs = [torch.empty((rows, B), device="cuda:0") if r else None for r in env._reward_reads()]
    rec("rew_vjp", timed(lambda: _native.rew_vjp(env.ENV_ID, env.dtype, B, rows, props, ctl, ref_strides, leaves, 1, B, g, 1, B, outs), reps),
        w * (2 * reads + nc + 1))
    out["rew_vjp"]["launch"] = _native.last_launch()
    gs = [None if o is None else o.t() for o in outs]
    rec("reverse_from_reward", timed(lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, None, gs, None), reps),
        w * (2 * A + S + reads))
    out["reverse_from_reward"]["launch"] = _native.last_launch()
    g_obs = torch.empty_like(obs).normal_()  # empty_like keeps the lane-major strides
    rec("reverse_from_obs", timed(lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, g_obs, None, None), reps),
        w * (2 * A + S + O))
    fwd = out["forward"]["fraction_of_peak"]
    for k in ("rew_trunc_term", "rew_vjp", "reverse_from_reward", "reverse_from_obs"):
        out[k]["of_forward_bandwidth"] = round(out[k]["fraction_of_peak"] / fwd, 3)
    out["total_ms"] = {"rew_vjp_plus_reverse_from_reward": round(out["rew_vjp"]["ms"] + out["reverse_from_reward"]["ms"], 4),
                       "reverse_from_obs": out["reverse_from_obs"]["ms"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "reward_vjp_cost.json"))
    a = ap.parse_args()
    from exciting_environments_amd import EnvironmentRegistry

    res = []
    for name, reg, control in (("pmsm", EnvironmentRegistry.PMSM, ("i_d", "i_q")), ("pendulum", EnvironmentRegistry.PENDULUM, ("theta",))):
        r = workload(name, reg, control, a.batch, a.steps, a.reps)
        print(json.dumps(r))
        res.append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
