#!/usr/bin/env python3
"""What a policy rollout costs per action row next to the routes that existed before it: pendulum and PMSM, Euler, fp32, B = 2^15,
K action rows of one solver step each, tanh networks with hidden widths (64, 64) and (16,):
  policy          one `vmap_sim_ahead_policy` (noise rows read, clip (-1, 1), state trajectory and applied actions written): one
                  launch of sim_policy_kernel
  open_loop       one `vmap_sim_ahead` of the same shape under "step" semantics with lane-major actions that exist up front (the
                  library's default plan): what the network inside the launch costs on top
  stepper_closed  the route a neural policy had before: the HIP-graph `Stepper` (graph=True), a one-step replay per step with the
                  same MLP as torch launches (addmm, tanh per hidden layer, add, clamp) writing the next action
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-up launches, then the median of 10 timed ones (device events around one launch; the stepper route by
the host clock around a window that ends in a device synchronise). Reported with each policy figure: the fused multiply-adds per lane
and action row, sum_l d_l d_{l-1}, and the fraction of the fp32 vector peak they amount to (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
FMAs / s). No test asserts a time.
usage: tools/policy_cost.py [--json FILE] [--B B] [--K N]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FMA_PEAK = 256 * 4 * 16 * 2.4e9  # fp32 FMA instructions x lanes / s of the whole chip (non-packed)
DEV = "cuda:0"
WARMUP, REPS = 3, 10
NETS = {"64x64": (64, 64), "16": (16,)}


def make(name, B, hidden):
    import torch
    from exciting_environments_amd import EnvironmentRegistry

    reg = {"pendulum": EnvironmentRegistry.PENDULUM, "pmsm": EnvironmentRegistry.PMSM}[name]
    env = reg.make(batch_size=B, dtype=torch.float32, device=DEV)
    env.sim_ahead_semantics = "step"
    _, state = env.vmap_reset()
    g = torch.Generator(device="cpu").manual_seed(3)
    if name == "pmsm":
        state.physical_state.omega_el = (torch.rand(B, generator=g) * 600).to(DEV)
        state.physical_state.epsilon = ((torch.rand(B, generator=g) - 0.5) * 6).to(DEV)
    else:
        state.physical_state.theta = ((torch.rand(B, generator=g) - 0.5) * 6).to(DEV)
    widths = (env._obs_dim(),) + tuple(hidden) + (env.action_dim,)
    W = [torch.randn(d, n, generator=g) / n ** 0.5 for n, d in zip(widths[:-1], widths[1:])]
    b = [(torch.rand(d, generator=g) - 0.5) * 0.2 for d in widths[1:]]
    return env, state, W, b, widths


def event_ms(fn):
    import torch

    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(float(t0.elapsed_time(t1)))
    return out


def host_ms(fn):
    import torch

    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def one(route, name, net, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import MLPPolicy, _native

    assert torch.cuda.is_available(), "policy_cost.py measures on a HIP device"
    env, state, W, b, widths = make(name, B, NETS[net])
    tau = env.tau
    if route == "policy":
        policy = MLPPolicy(W, b, "tanh")
        noise = env.new_actions_buffer(K)
        noise.normal_(0.0, 0.1)
        fn = lambda: env.vmap_sim_ahead_policy(state, policy, K, tau, tau, noise=noise)
        ms = event_ms(fn)
        launch = env.last_policy_launch
    elif route == "open_loop":
        acts = env.new_actions_buffer(K)
        acts.uniform_(-1, 1)
        env.trajectory_placement = "off"  # fresh allocations like the policy call's: the same memory behaviour on both sides
        env.trajectory_pool = False
        fn = lambda: env.vmap_sim_ahead(state, acts, tau, tau)
        ms = event_ms(fn)
        launch = _native.last_launch()
    else:  # stepper_closed: one-step replays with the MLP in torch between them
        st = env.make_stepper(n_steps=1, graph=True)
        st.reset(state)
        Wt = [w.t().contiguous().to(DEV) for w in W]
        bd = [v.to(DEV) for v in b]
        noise = (torch.randn(K, B, env.action_dim) * 0.1).to(DEV)
        obs0 = torch.zeros(B, env._obs_dim(), device=DEV)  # the first action only; every later one reads the step's observation

        def fn():
            ob = obs0
            for k in range(K):
                x = ob
                for l in range(len(Wt) - 1):
                    x = torch.tanh(torch.addmm(bd[l], x, Wt[l]))
                x = torch.addmm(bd[-1], x, Wt[-1])
                torch.clamp(x + noise[k], -1.0, 1.0, out=st.actions[0])
                ob = st.run()[0][0]

        ms = host_ms(fn)
        launch = "Stepper(graph=True), one step per replay + the MLP in torch"
    med = statistics.median(ms)
    fmas = sum(n * d for n, d in zip(widths[:-1], widths[1:]))
    r = dict(route=route, env=name, net=net, widths=list(widths), B=B, K=K, launch=launch, ms_median=med, ms_min=min(ms), ms_max=max(ms),
             us_per_row=med * 1e3 / K)
    if route == "policy":
        r["fma_per_lane_row"] = fmas
        r["fraction_of_fp32_fma_peak"] = fmas * B * K / (med * 1e-3) / FMA_PEAK
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--B", type=int, default=1 << 15)
    ap.add_argument("--K", type=int, default=1000, help="action rows")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=4, metavar=("ROUTE", "ENV", "NET", "B"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], a.one[2], int(a.one[3]), a.K)))
        return 0
    jobs = []
    for name in ("pendulum", "pmsm"):
        jobs.append(("open_loop", name, "16"))
        for net in NETS:
            jobs += [("policy", name, net), ("stepper_closed", name, net)]
    results = []
    for route, name, net in jobs:  # one after the other, each under its own time limit; the first failure ends the session
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--K", str(a.K), "--one", route, name, net,
               str(a.B)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} {net}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(fp32_fma_peak_per_s=FMA_PEAK, complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        if route == "open_loop":
            r["net"] = None  # no network in this route
        results.append(r)
        frac = f"  {r['fraction_of_fp32_fma_peak']:.3f} of the fp32 FMA peak" if "fraction_of_fp32_fma_peak" in r else ""
        print(f"{name:9s} B={a.B:7d} {route:15s} net {str(r['net']):6s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
              f"{r['us_per_row']:8.3f} us / row{frac}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(fp32_fma_peak_per_s=FMA_PEAK, complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
