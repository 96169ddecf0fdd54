#!/usr/bin/env python3
"""What the parameter gradient of a policy rollout costs on each route: pendulum and PMSM, Euler, fp32, a tanh
network with hidden layers (64, 64) and (16,), noise rows and clip (-1, 1), one step per action row, a loss on the observations, at
B = 2^15 with K = 1000 action rows: the rows of tools/policy_vjp_cost.py.
  torch            the torch contraction alone: `torch.autograd.grad(policy.torch_forward(rows), params, g_noise)` in the chunks of
                   `_policy_vjp.PARAM_CHUNK`, on the stored observation rows and the grad_raw of one reverse launch
  fused            the fused entry alone: one `vmap_policy_param_grads` on the same arrays (policy_param_grad_kernel and
                   policy_param_grad_reduce_kernel)
  backward_torch   the whole backward, `vmap_sim_ahead_policy_vjp(..., param_grads="torch")`
  backward_fused   the whole backward, `vmap_sim_ahead_policy_vjp(..., param_grads="fused")`
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-ups, then the median of 10, device events around one call.
usage: tools/policy_param_grad_cost.py [--json FILE] [--B N] [--K N]"""
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

from policy_vjp_cost import CLIP, NETS, event_ms, make  # noqa: E402  (the same environments, networks and timing loop)

ROUTES = ("torch", "fused", "backward_torch", "backward_fused")


def one(route, name, net, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import _native, _policy_vjp

    assert torch.cuda.is_available(), "policy_param_grad_cost.py measures on a HIP device"
    env, state, policy = make(name, B, NETS[net])
    tau = env.tau
    A, OW = env.action_dim, env._obs_dim()
    noise = env.new_actions_buffer(K)
    noise.normal_().mul_(0.3)
    obs, states, last, actions = env.vmap_sim_ahead_policy(state, policy, K, tau, tau, noise=noise, clip=CLIP)
    g_obs = torch.empty_like(obs).normal_()  # lane-major like obs: read in place
    vjp = lambda pg: env.vmap_sim_ahead_policy_vjp(policy, obs, states, actions, tau, tau, clip=CLIP, grad_obs=g_obs, param_grads=pg)
    r = dict(route=route, env=name, net=net, B=B, K=K, n_params=int(policy.params.numel()))
    if route.startswith("backward_"):
        ms = event_ms(lambda: vjp(route[len("backward_"):]))
        r["launch"] = env.last_policy_vjp_launch + " + " + ("the parameter contraction in torch" if route == "backward_torch" else _native.last_launch())
    else:
        _, g_noise, _ = vjp(False)
        if route == "fused":
            ms = event_ms(lambda: env.vmap_policy_param_grads(policy, obs, g_noise, tau, tau))
            r["launch"] = _native.last_launch()
        else:
            params = policy.params.detach()
            rows_k = obs[:, 0:K, :]  # the observation rows of the action rows (one step per action row)
            chunk = _policy_vjp.PARAM_CHUNK
            bc = min(B, chunk)
            kc = max(1, chunk // bc)

            def contraction():  # the statements of _policy_vjp_launch's torch route
                out = torch.zeros_like(params)
                with torch.enable_grad():
                    p = params.clone().requires_grad_()
                    for b0 in range(0, B, bc):
                        for k0 in range(0, K, kc):
                            x = rows_k[b0:b0 + bc, k0:k0 + kc].reshape(-1, OW)
                            g = g_noise[b0:b0 + bc, k0:k0 + kc].reshape(-1, A)
                            out += torch.autograd.grad(policy.torch_forward(x, p), p, g)[0]
                return out

            ms = event_ms(contraction)
            r["launch"] = "the parameter contraction in torch"
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
    jobs = [(route, name, net, a.B, a.K) for name in ("pendulum", "pmsm") for net in NETS for route in ROUTES]
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
        print(f"{name:9s} {net:6s} B={B:8d} K={K:5d} {route:15s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
              f"{r['us_per_row']:8.3f} us / row   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
