#!/usr/bin/env python3
"""What the gradient through a closed-loop trajectory costs next to the launches around it: pendulum and PMSM, Euler, fp32, one
broadcast gain set with integral action and clip (-1, 1), one step per action row, a loss on the observations (grad_obs is the one
cotangent group), at B = 2^15 with K = 1000 action rows and at B = 2^22 with K = 128 (pendulum) / K = 100 (PMSM, the benchmark's shape).
  backward    one `vmap_sim_ahead_feedback_vjp` on a stored forward: the whole launch sequence of excenv_sim_feedback_vjp — the
              integrator pre-pass, sim_feedback_vjp_kernel, the gain-gradient kernel once per gain set and the batch sums
  forward     the closed-loop forward of the same shape (`vmap_sim_ahead_feedback`, states and actions written)
  open_vjp    the open-loop `vmap_sim_ahead_vjp` of the same shape on the returned actions, "step" semantics, envs_per_lane = 1:
              what the transposed policy, the integrator's cotangent and the gain gradients cost on top
  chain       B = 2^15, K = 100 only: what one had to do before — `.backward()` through a chain of K differentiable `vmap_step`
              calls with the same policy in torch (one step_vjp launch plus the policy's torch launches per step); the graph is
              built outside the timed window
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-ups, then the median of 10 (device events around one call; `chain` by the host clock around a
window that ends in a device synchronise). The backward's algorithmic bytes per environment and action row are
excenv_sim_feedback_vjp_bytes; their fraction of the 8 TB/s HBM peak is reported.
usage: tools/feedback_vjp_cost.py [--json FILE] [--small B] [--large B] [--K N] [--K-large-pendulum N] [--K-large-pmsm N]"""
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
CLIP = (-1.0, 1.0)


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
    igain = (torch.randn(env.action_dim, OW, generator=g) * 0.25 / OW ** 0.5 / env.tau / 100).to(DEV)
    return env, state, gain, igain


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


def one(route, name, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import _native

    assert torch.cuda.is_available(), "feedback_vjp_cost.py measures on a HIP device"
    env, state, gain, igain = make(name, B)
    tau = env.tau
    S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
    forward = lambda: env.vmap_sim_ahead_feedback(state, gain, K, tau, tau, integral_gain=igain, clip=CLIP)
    r = dict(route=route, env=name, B=B, K=K)
    if route == "forward":
        ms = event_ms(forward)
        r["launch"] = env.last_feedback_launch
    elif route in ("backward", "open_vjp"):
        obs, states, last, actions, z = forward()
        g_obs = torch.empty_like(obs).normal_()  # lane-major like obs: read in place
        if route == "backward":
            fn = lambda: env.vmap_sim_ahead_feedback_vjp(state, gain, obs, states, actions, tau, tau, integral_gain=igain, clip=CLIP,
                                                         grad_obs=g_obs)
            ms = event_ms(fn)
            r["launch"] = env.last_feedback_vjp_launch + " (+ pre-pass, gain gradients, batch sums)"
            r["bytes_per_env_row"] = int(_native.lib().excenv_sim_feedback_vjp_bytes(env.ENV_ID, _native.dtype_id(env.dtype), 0, 1, 1, 1, 0, 0))
            r["fraction_of_hbm_peak"] = r["bytes_per_env_row"] * B * K / (statistics.median(ms) * 1e-3) / PEAK
        else:
            env.launch_opts = _native.launch_opts(envs_per_lane=1)
            fn = lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, g_obs)
            ms = event_ms(fn)
            r["launch"] = env.last_vjp_launch
    else:  # chain: the policy in torch around differentiable steps; only .backward() is timed
        env.differentiable = True
        g = gain.clone().requires_grad_(True)
        gi = igain.clone().requires_grad_(True)
        w = torch.randn(B, OW, device=DEV)

        def build():
            ob = env.generate_observation(state, env.env_properties)
            s, zz, loss = state, torch.zeros(B, A, device=DEV), 0.0
            for _ in range(K):
                acc = zz + ob @ g.t()
                a = torch.where((acc > CLIP[0]) & (acc < CLIP[1]), acc, acc.detach().clamp(*CLIP))
                zs = zz + tau * (ob @ gi.t())
                zz = torch.where((zs > CLIP[0]) & (zs < CLIP[1]), zs, zs.detach().clamp(*CLIP))
                ob, s = env.vmap_step(s, a)
                loss = loss + (ob * w).sum()
            return loss

        ms = []
        for i in range(WARMUP + REPS):
            loss = build()
            g.grad = gi.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        r["launch"] = env.last_step_vjp_launch + " per step + the policy's torch backward"
    med = statistics.median(ms)
    r.update(ms_median=med, ms_min=min(ms), ms_max=max(ms), us_per_row=med * 1e3 / K)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--small", type=int, default=1 << 15)
    ap.add_argument("--large", type=int, default=1 << 22)
    ap.add_argument("--K", type=int, default=1000, help="action rows at the small batch size")
    ap.add_argument("--K-large-pendulum", type=int, default=128)
    ap.add_argument("--K-large-pmsm", type=int, default=100)
    ap.add_argument("--K-chain", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=4, metavar=("ROUTE", "ENV", "B", "K"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], int(a.one[2]), int(a.one[3]))))
        return 0
    jobs = []
    for name in ("pendulum", "pmsm"):
        for B, K in ((a.small, a.K), (a.large, a.K_large_pendulum if name == "pendulum" else a.K_large_pmsm)):
            jobs += [("backward", name, B, K), ("forward", name, B, K), ("open_vjp", name, B, K)]
        jobs.append(("chain", name, a.small, a.K_chain))
    results = []
    for route, name, B, K in jobs:  # one after the other, each under its own time limit; the first failure ends the session
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", route, name, str(B), str(K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} B={B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(peak_bytes_per_s=PEAK, complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        results.append(r)
        frac = f"  {r['fraction_of_hbm_peak']:.3f} of the HBM peak" if "fraction_of_hbm_peak" in r else ""
        print(f"{name:9s} B={B:8d} K={K:5d} {route:9s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
              f"{r['us_per_row']:8.3f} us / row{frac}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(peak_bytes_per_s=PEAK, complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
