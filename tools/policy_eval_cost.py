#!/usr/bin/env python3
"""What the update step of an on-policy trainer costs on the rows of an episode rollout: pendulum and PMSM,
Euler, fp32, a tanh network with hidden layers (64, 64) and (16,), `vmap_rollout_episodes` at B = 2^15 with K = 1000 action rows
(the rollout of tools/episode_cost.py). On its views, read in place:
  eval_fused       `vmap_policy_eval(policy, ro.observations)`, no graph: one launch of policy_eval_kernel over all K + 1 rows
  eval_torch       `policy.torch_forward(ro.observations)` without a graph, in chunks of `_policy_vjp.PARAM_CHUNK` samples (the chunks
                   of the torch route of the parameter gradient: one pass would materialise B (K + 1) x 64 activations per layer)
  evalbwd_fused    forward and backward of a sum: `vmap_policy_eval(...).sum().backward()` with `policy.params` requiring grad
                   (policy_eval_kernel, then policy_param_grad_kernel and its reduction)
  evalbwd_torch    the same through `policy.torch_forward` in those chunks, `backward()` per chunk
  gae_fused        `vmap_gae(ro.reward, value, 0.99, 0.95, ro.terminated, ro.reset)`: one launch of gae_kernel
  gae_torch        the same recurrence as a torch host loop over the K rows of the lane-major views
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-ups, then the median of 10, device events around one call.
usage: tools/policy_eval_cost.py [--json FILE] [--B N] [--K N]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from episode_cost import MAX_EPISODE_STEPS, make  # noqa: E402  (the same environments, networks and rollout)
from policy_cost import NETS, event_ms  # noqa: E402

ROUTES = ("eval_fused", "eval_torch", "evalbwd_fused", "evalbwd_torch", "gae_fused", "gae_torch")
GAMMA, LAM = 0.99, 0.95


def one(route, name, net, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import MLPPolicy, _native, _policy_vjp

    assert torch.cuda.is_available(), "policy_eval_cost.py measures on a HIP device"
    env, state, reset_state, W, b, widths, steps = make(name, B, NETS[net])
    tau = env.tau
    policy = MLPPolicy(W, b, "tanh", device=env.device, dtype=env.dtype)
    noise = env.new_actions_buffer(K)
    noise.normal_(0.0, 0.1)
    ro = env.vmap_rollout_episodes(state, policy, K, tau, reset_state, noise=noise, max_episode_steps=MAX_EPISODE_STEPS, episode_steps=steps)
    obs = ro.observations  # [B, K + 1, OW] over [K + 1][OW][B]
    OW = widths[0]
    r = dict(route=route, env=name, net=net, B=B, K=K, n_params=int(policy.params.numel()), reset_share=float(ro.reset.float().mean()))
    chunk = _policy_vjp.PARAM_CHUNK
    bc = min(B, chunk)
    kc = max(1, chunk // bc)
    if route == "eval_fused":
        with torch.no_grad():
            ms = event_ms(lambda: env.vmap_policy_eval(policy, obs))
        r["launch"] = _native.last_launch()
    elif route == "eval_torch":
        def forward():
            out = torch.empty((B, K + 1, widths[-1]), dtype=env.dtype, device=env.device)
            with torch.no_grad():
                for b0 in range(0, B, bc):
                    for k0 in range(0, K + 1, kc):
                        x = obs[b0:b0 + bc, k0:k0 + kc]
                        out[b0:b0 + bc, k0:k0 + kc] = policy.torch_forward(x.reshape(-1, OW)).reshape(x.shape[0], x.shape[1], -1)
            return out

        ms = event_ms(forward)
        r["launch"] = "policy.torch_forward in chunks"
    elif route == "evalbwd_fused":
        policy.params.requires_grad_()

        def both():
            policy.params.grad = None
            env.vmap_policy_eval(policy, obs).sum().backward()

        ms = event_ms(both)
        r["launch"] = "policy_eval_kernel + policy_param_grad_kernel"
    elif route == "evalbwd_torch":
        policy.params.requires_grad_()

        def both():
            policy.params.grad = None
            for b0 in range(0, B, bc):
                for k0 in range(0, K + 1, kc):
                    policy.torch_forward(obs[b0:b0 + bc, k0:k0 + kc].reshape(-1, OW)).sum().backward()

        ms = event_ms(both)
        r["launch"] = "policy.torch_forward and torch's backward in chunks"
    else:
        value = torch.empty((K + 1, B), dtype=env.dtype, device=env.device).normal_().t()  # lane-major like the rollout's rows
        if route == "gae_fused":
            ms = event_ms(lambda: env.vmap_gae(ro.reward, value, GAMMA, LAM, terminated=ro.terminated, reset=ro.reset))
            r["launch"] = _native.last_launch()
        else:
            rew, val, term, cut = ro.reward.t(), value.t(), ro.terminated.t(), ro.reset.t()  # [K][B] rows
            g, gl = GAMMA, GAMMA * LAM

            def loop():
                adv = torch.empty_like(rew)
                carry = torch.zeros_like(rew[0])
                zero = torch.zeros_like(carry)
                for n in range(K - 1, -1, -1):
                    boot = torch.where(term[n], zero, val[n + 1])
                    delta = rew[n] + g * boot - val[n]
                    run = torch.where(term[n], delta, delta + gl * carry)
                    carry = torch.where(cut[n], zero, run)
                    adv[n] = carry
                return adv, torch.where(cut, val[:K], adv + val[:K])

            ms = event_ms(loop)
            r["launch"] = "torch host loop over K rows"
    med = statistics.median(ms)
    r.update(ms_median=med, ms_min=min(ms), ms_max=max(ms), us_per_row=med * 1e3 / K)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--B", type=int, default=1 << 15)
    ap.add_argument("--K", type=int, default=1000, help="action rows")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=5, metavar=("ROUTE", "ENV", "NET", "B", "K"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], a.one[2], int(a.one[3]), int(a.one[4]))))
        return 0
    # the GAE rows need no network: once per environment
    jobs = [(route, name, net, a.B, a.K) for name in ("pendulum", "pmsm") for net in NETS for route in ROUTES
            if not (route.startswith("gae_") and net != "16")]
    results = []
    for route, name, net, B, K in jobs:  # one after the other, each under its own time limit; the first failure ends the session
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", route, name, net, str(B), str(K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} {net} B={B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        results.append(r)
        print(f"{name:9s} {net:6s} B={B:8d} K={K:5d} {route:14s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
              f"{r['us_per_row']:8.3f} us / row   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
