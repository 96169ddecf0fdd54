#!/usr/bin/env python3
"""What the gradient through a policy rollout costs next to the launches around it: pendulum and PMSM, Euler, fp32, a tanh network
with hidden layers (64, 64) and (16,), noise rows and clip (-1, 1), one step per action row, a loss on the observations (grad_obs is
the one cotangent group), at B = 2^15 with K = 1000 action rows.
  reverse         one `vmap_sim_ahead_policy_vjp(..., param_grads=False)` on a stored forward: the one launch of sim_policy_vjp_kernel
  reverse_params  the same with the parameter contraction in torch behind it (`param_grads=True`)
  forward         the policy rollout of the same shape (`vmap_sim_ahead_policy`, states and actions written)
  chain           K = 100 only: what one had to do before — `.backward()` through a chain of K differentiable `vmap_step` calls with
                  the network in torch (one step_vjp launch plus the network's torch launches per step); the graph is built outside
                  the timed window
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-ups, then the median of 10 (device events around one call; `chain` by the host clock around a
window that ends in a device synchronise). The reverse launch's algorithmic bytes per environment and action row are
excenv_sim_policy_vjp_bytes; their fraction of the 8 TB/s HBM peak is reported.
usage: tools/policy_vjp_cost.py [--json FILE] [--B N] [--K N] [--K-chain N]"""
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
NETS = {"64x64": (64, 64), "16": (16,)}


def make(name, B, hidden):
    import torch
    from exciting_environments_amd import EnvironmentRegistry, MLPPolicy

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
    return env, state, MLPPolicy(W, b, "tanh", device=DEV, dtype=torch.float32)


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


def one(route, name, net, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import _native

    assert torch.cuda.is_available(), "policy_vjp_cost.py measures on a HIP device"
    env, state, policy = make(name, B, NETS[net])
    tau = env.tau
    A, OW = env.action_dim, env._obs_dim()
    noise = env.new_actions_buffer(K)
    noise.normal_().mul_(0.3)
    forward = lambda: env.vmap_sim_ahead_policy(state, policy, K, tau, tau, noise=noise, clip=CLIP)
    r = dict(route=route, env=name, net=net, B=B, K=K)
    if route == "forward":
        ms = event_ms(forward)
        r["launch"] = env.last_policy_launch
    elif route in ("reverse", "reverse_params"):
        obs, states, last, actions = forward()
        g_obs = torch.empty_like(obs).normal_()  # lane-major like obs: read in place
        fn = lambda: env.vmap_sim_ahead_policy_vjp(policy, obs, states, actions, tau, tau, clip=CLIP, grad_obs=g_obs,
                                                   param_grads=route == "reverse_params")
        ms = event_ms(fn)
        r["launch"] = env.last_policy_vjp_launch + (" + the parameter contraction in torch" if route == "reverse_params" else "")
        if route == "reverse":
            r["bytes_per_env_row"] = int(_native.lib().excenv_sim_policy_vjp_bytes(env.ENV_ID, _native.dtype_id(env.dtype), 0, 1, 1, 0, 0, 0))
            r["fraction_of_hbm_peak"] = r["bytes_per_env_row"] * B * K / (statistics.median(ms) * 1e-3) / PEAK
    else:  # chain: the network in torch around differentiable steps; only .backward() is timed
        env.differentiable = True
        p = policy.params.clone().requires_grad_(True)
        w = torch.randn(B, OW, device=DEV)

        def build():
            ob = env.generate_observation(state, env.env_properties)
            s, loss = state, 0.0
            for k in range(K):
                raw = noise[:, k] + policy.torch_forward(ob, p)
                a = torch.where((raw > CLIP[0]) & (raw < CLIP[1]), raw, raw.detach().clamp(*CLIP))
                ob, s = env.vmap_step(s, a)
                loss = loss + (ob * w).sum()
            return loss

        ms = []
        for i in range(WARMUP + REPS):
            loss = build()
            p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss.backward()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        r["launch"] = env.last_step_vjp_launch + " per step + the network's torch backward"
    med = statistics.median(ms)
    r.update(ms_median=med, ms_min=min(ms), ms_max=max(ms), us_per_row=med * 1e3 / K)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--B", type=int, default=1 << 15)
    ap.add_argument("--K", type=int, default=1000, help="action rows of the launches")
    ap.add_argument("--K-chain", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=5, metavar=("ROUTE", "ENV", "NET", "B", "K"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], a.one[2], int(a.one[3]), int(a.one[4]))))
        return 0
    jobs = []
    for name in ("pendulum", "pmsm"):
        for net in NETS:
            jobs += [("reverse", name, net, a.B, a.K), ("reverse_params", name, net, a.B, a.K), ("forward", name, net, a.B, a.K),
                     ("chain", name, net, a.B, a.K_chain)]
    results = []
    for route, name, net, B, K in jobs:  # one after the other, each under its own time limit; the first failure ends the session
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", route, name, net, str(B), str(K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} {net} B={B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(peak_bytes_per_s=PEAK, complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        results.append(r)
        frac = f"  {r['fraction_of_hbm_peak']:.3f} of the HBM peak" if "fraction_of_hbm_peak" in r else ""
        print(f"{name:9s} {net:6s} B={B:8d} K={K:5d} {route:14s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
              f"{r['us_per_row']:8.3f} us / row{frac}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(peak_bytes_per_s=PEAK, complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
