#!/usr/bin/env python3
"""What a closed-loop trajectory costs per solver step next to the routes that existed before it: pendulum and PMSM, Euler, fp32,
K = 1000 action rows of one step each, at B = 2^15 and B = 2^22 — except PMSM at B = 2^22, which runs K = 100 (the benchmark's shape):
1000 rows of 2^22 PMSM environments would be 285 GB of trajectories (the pendulum's are 84 GB and run as asked).
  feedback    one `vmap_sim_ahead_feedback` (one broadcast gain set, clip (-1, 1), state trajectory and applied actions written):
              one launch of sim_feedback_kernel
  open_loop   one `vmap_sim_ahead` of the same shape under "step" semantics with lane-major actions that exist up front (the
              library's default plan): what the policy inside the launch costs on top
  stepper     B = 2^15 only: the HIP-graph `Stepper` (graph=True), per step — `chain`: one replay of a 100-step chain with fixed
              actions (no controller at all: the floor of the host route); `closed`: a one-step replay per step with the same affine
              policy as two torch launches (addmm, clamp) writing the next action, which is what a closed loop had to do
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-up launches, then the median of 10 timed ones (device events around one launch; the stepper routes
by the host clock around a window that ends in a device synchronise). Bytes per environment-step of the feedback launch:
w (OW + S + A); its fraction of the 8 TB/s HBM peak is reported at B = 2^22.
usage: tools/feedback_cost.py [--json FILE] [--small B] [--large B] [--K N] [--K-large-pmsm N]"""
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

PEAK = 8.0e12  # bytes / s
DEV = "cuda:0"
WARMUP, REPS = 3, 10


def make(name, B):
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
    OW = env._obs_dim()
    gain = (torch.randn(env.action_dim, OW, generator=g) * 0.5 / OW ** 0.5).to(DEV)
    return env, state, gain


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


def one(route, name, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import _native

    assert torch.cuda.is_available(), "feedback_cost.py measures on a HIP device"
    env, state, gain = make(name, B)
    tau = env.tau
    steps = K
    if route == "feedback":
        fn = lambda: env.vmap_sim_ahead_feedback(state, gain, K, tau, tau)
        ms = event_ms(fn)
        launch = env.last_feedback_launch
    elif route == "open_loop":
        acts = env.new_actions_buffer(K)
        acts.uniform_(-1, 1)
        env.trajectory_placement = "off"  # fresh allocations like the feedback call's: the same memory behaviour on both sides
        env.trajectory_pool = False
        fn = lambda: env.vmap_sim_ahead(state, acts, tau, tau)
        ms = event_ms(fn)
        launch = _native.last_launch()
    elif route == "stepper_chain":
        steps = 100
        st = env.make_stepper(n_steps=steps, graph=True)
        st.reset(state)
        st.actions.uniform_(-1, 1)
        ms = host_ms(st.run)
        launch = "Stepper(graph=True), 100-step chain"
    else:  # stepper_closed: one-step replays with the affine policy in torch between them
        st = env.make_stepper(n_steps=1, graph=True)
        st.reset(state)
        gt = gain.t().contiguous()
        obs0 = torch.zeros(B, env._obs_dim(), device=DEV)  # the first action only; every later one reads the step's observation

        def fn():
            ob = obs0
            for _ in range(K):
                torch.clamp(torch.mm(ob, gt), -1.0, 1.0, out=st.actions[0])
                ob = st.run()[0][0]

        ms = host_ms(fn)
        launch = "Stepper(graph=True), one step per replay + torch.mm / clamp"
    med = statistics.median(ms)
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    r = dict(route=route, env=name, B=B, K=K, steps=steps, launch=launch, ms_median=med, ms_min=min(ms), ms_max=max(ms),
             us_per_step=med * 1e3 / steps)
    if route in ("feedback", "open_loop"):
        r["bytes_per_env_step"] = 4 * (OW + S + A)  # feedback: obs, states, applied action out; open loop: the action in instead
        r["fraction_of_hbm_peak"] = r["bytes_per_env_step"] * B * steps / (med * 1e-3) / PEAK
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--small", type=int, default=1 << 15)
    ap.add_argument("--large", type=int, default=1 << 22)
    ap.add_argument("--K", type=int, default=1000, help="action rows")
    ap.add_argument("--K-large-pmsm", type=int, default=100, help="action rows of PMSM at the large batch size (memory)")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=3, metavar=("ROUTE", "ENV", "B"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], int(a.one[2]), a.K)))
        return 0
    jobs = []
    for name in ("pendulum", "pmsm"):
        for B in (a.small, a.large):
            jobs += [("feedback", name, B), ("open_loop", name, B)]
        jobs += [("stepper_chain", name, a.small), ("stepper_closed", name, a.small)]
    results = []
    for route, name, B in jobs:  # one after the other, each under its own time limit; the first failure ends the session
        K = a.K_large_pmsm if (name == "pmsm" and B == a.large and a.large != a.small) else a.K
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--K", str(K), "--one", route, name, str(B)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} B={B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(peak_bytes_per_s=PEAK, complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        results.append(r)
        frac = f"  {r['fraction_of_hbm_peak']:.3f} of the HBM peak" if "fraction_of_hbm_peak" in r and B == a.large else ""
        print(f"{name:9s} B={B:8d} {route:15s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
              f"{r['us_per_step']:8.3f} us / step{frac}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(peak_bytes_per_s=PEAK, complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
