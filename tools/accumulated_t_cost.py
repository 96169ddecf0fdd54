#!/usr/bin/env python3
"""What the accumulated-time clock costs: "ahead" against "ahead_accumulated_t" (EXCENV_SEM_AHEAD_ACCUMULATED_T) in one process, on
the SAME buffers (lane-major actions [K][A][B], lane-major observation and state trajectories), alternating the two semantics call
by call and timing each launch with HIP events. B = 2^22, K = 100. Prints one JSON line per workload (median kernel milliseconds
of each semantics and their ratio) and writes them to --json.
usage (GPU box): python tools/accumulated_t_cost.py [--calls 30] [--json OUT]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "exciting-environments_amd")]
import exciting_environments_amd as ex  # noqa: E402
from exciting_environments_amd import EnvironmentRegistry, _native  # noqa: E402

WORKLOADS = [("pmsm", "euler", torch.float32), ("pmsm", "tsit5", torch.float32), ("pendulum", "euler", torch.float32),
             ("mass_spring_damper", "tsit5", torch.float64)]
REG = {"pmsm": EnvironmentRegistry.PMSM, "pendulum": EnvironmentRegistry.PENDULUM,
       "mass_spring_damper": EnvironmentRegistry.MASS_SPRING_DAMPER}


def run(name, solver, dtype, B, K, calls):
    solv = {"euler": ex.Euler(), "tsit5": ex.Tsit5()}[solver]
    env = REG[name].make(batch_size=B, solver=solv, dtype=dtype, device="cuda:0")
    dev, S, A, OW = env.device, env.physical_state_dim, env.action_dim, env._obs_dim()
    _, state = env.vmap_reset()
    g = torch.Generator(device=dev).manual_seed(1)
    if name == "pmsm":  # stable-region speeds
        state.physical_state.omega_el = torch.rand(B, generator=g, device=dev, dtype=dtype) * 600
    st_in = [getattr(state.physical_state, n).contiguous() for n in env.STATE_FIELDS]
    actions = torch.rand((K, A, B), generator=g, device=dev, dtype=dtype) * 2 - 1  # lane-major [K][A][B]
    props, _keep = env._props_for(env.env_properties, B)
    obs = torch.empty((K + 1, OW, B), dtype=dtype, device=dev)
    straj = [torch.empty((K + 1, B), dtype=dtype, device=dev) for _ in range(S)]
    last = [torch.empty(B, dtype=dtype, device=dev) for _ in range(S)]
    times = {_native.SEM_AHEAD: [], _native.SEM_AHEAD_ACCUMULATED_T: []}
    launches = {}
    for i in range(calls + 2):
        for sem in times:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _native.sim_ahead(env.ENV_ID, env._solver.id, dtype, B, K, 1, props, None, float(env.tau), float(env.tau), st_in,
                              actions, _native.LAYOUT_LANE_MAJOR, obs, straj, _native.LAYOUT_LANE_MAJOR, last, sem)
            e1.record()
            launches[sem] = _native.last_launch()
            torch.cuda.synchronize()
            if i >= 2:  # warm-up
                times[sem].append(e0.elapsed_time(e1))
    ah, acc = (statistics.median(times[s]) for s in (_native.SEM_AHEAD, _native.SEM_AHEAD_ACCUMULATED_T))
    return {"workload": f"{name} {solver} {'fp32' if dtype is torch.float32 else 'fp64'}", "B": B, "K": K, "calls": calls,
            "ahead_ms": round(ah, 4), "accumulated_t_ms": round(acc, 4), "ratio": round(acc / ah, 4),
            "ahead_min_ms": round(min(times[_native.SEM_AHEAD]), 4),
            "accumulated_t_min_ms": round(min(times[_native.SEM_AHEAD_ACCUMULATED_T]), 4),
            "launch_ahead": launches[_native.SEM_AHEAD], "launch_accumulated_t": launches[_native.SEM_AHEAD_ACCUMULATED_T]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--batch", type=int, default=22, help="log2 of the batch size")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for name, solver, dtype in WORKLOADS:
        rows.append(run(name, solver, dtype, 1 << a.batch, 100, a.calls))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
