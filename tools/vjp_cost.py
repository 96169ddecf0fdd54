#!/usr/bin/env python3
"""What the reverse launch costs next to the forward launch, over the same buffers in one process: PMSM Euler fp32 and pendulum
Euler fp32 at B = 2^20, K = 100 (options below). Per workload: the forward launch (vmap_sim_ahead into the outputs of a first
call), the backward launch with all three cotangent groups present and with the last_state cotangent alone — median of the timed
launches after warm-up, algorithmic bytes (forward w (A + O + S), backward w (2A + 2S + O) resp. w (2A + S) per env-step) and the
achieved fraction of the 8 TB/s HBM peak. The yardstick for the backward is the forward's bandwidth of the same run. Also: the
cost of bringing a row-major observation cotangent (what autograd hands back after a select / sum) into lane-major order.
usage: tools/vjp_cost.py [--batch B] [--steps K] [--reps N] [--json FILE]"""
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


def workload(name, reg, B, K, reps):
    from exciting_environments_amd import _native

    env = reg.make(batch_size=B, dtype=torch.float32, device="cuda:0")
    _, state = env.vmap_reset()
    if name == "pmsm":
        state.physical_state.omega_el = torch.rand(B, device="cuda:0") * 600
        state.physical_state.epsilon = (torch.rand(B, device="cuda:0") - 0.5) * 6
    actions = env.new_actions_buffer(K)
    actions.copy_((torch.rand(B, K, env.action_dim, device="cuda:0") - 0.5) * 1.5)
    tau = env.tau
    trip = env.vmap_sim_ahead(state, actions, tau, tau)
    obs, states, last = trip
    S, A, O = env.physical_state_dim, env.action_dim, obs.shape[-1]
    rows = K + 1
    g_obs = torch.empty_like(obs).normal_()  # empty_like keeps the lane-major strides
    g_states = [torch.empty_like(getattr(states.physical_state, n)).normal_() for n in env.STATE_FIELDS]
    g_last = [torch.randn(B, device="cuda:0") for _ in range(S)]
    assert tuple(g_obs.stride()) == tuple(obs.stride())
    w = 4
    out = {"workload": f"{name} euler fp32", "B": B, "K": K}

    def rec(key, ms, bytes_per_step):
        total = bytes_per_step * B * K
        out[key] = {"ms": round(ms, 4), "bytes_per_env_step": bytes_per_step, "gbytes": round(total / 1e9, 3),
                    "fraction_of_peak": round(total / (ms * 1e-3) / PEAK, 4)}

    rec("forward", timed(lambda: env.vmap_sim_ahead(state, actions, tau, tau, out=trip), reps), w * (A + O + S))
    rec("backward_all_cotangents",
        timed(lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, g_obs, g_states, g_last), reps), w * (2 * A + 2 * S + O))
    out["backward_all_cotangents"]["launch"] = _native.last_launch()
    rec("backward_last_state_only",
        timed(lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, None, None, g_last), reps), w * (2 * A + S))
    fwd = out["forward"]["fraction_of_peak"]
    for k in ("backward_all_cotangents", "backward_last_state_only"):
        out[k]["of_forward_bandwidth"] = round(out[k]["fraction_of_peak"] / fwd, 3)
    # a row-major cotangent must be brought into lane-major order first
    g_rm = torch.randn(B, rows, O, device="cuda:0")
    out["row_major_obs_cotangent_copy_ms"] = round(timed(lambda: env._lane_major(g_rm, (B, rows, O), (1, O * B, B)), reps), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from exciting_environments_amd import EnvironmentRegistry

    res = []
    for name, reg in (("pmsm", EnvironmentRegistry.PMSM), ("pendulum", EnvironmentRegistry.PENDULUM)):
        r = workload(name, reg, a.batch, a.steps, max(10, a.reps))
        print(json.dumps(r))
        res.append(r)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
