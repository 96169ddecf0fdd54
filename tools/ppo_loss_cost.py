#!/usr/bin/env python3
"""What the PPO objective costs on the rows of an episode rollout: pendulum (A = 1) and PMSM (A = 2), Euler, fp32, a
tanh network with one hidden layer of 16, `vmap_rollout_episodes` at B = 2^15 with K = 1000 action rows (the rollout of
tools/episode_cost.py). On its views and on those of `vmap_policy_eval` / `vmap_gae`, read in place:
  logp_fused      `vmap_gaussian_logp(mean_old, sample, log_std)`: one launch of gaussian_logp_kernel
  logp_torch      the same log-probability as an elementwise torch expression on the views, no graph
  loss_fused      `vmap_ppo_loss(...)` without a graph: ppo_loss_kernel and its reduction, then the scalar ops of the fields
  loss_torch      the clipped surrogate, value loss, entropy, approximate KL and clip fraction as elementwise torch, no graph
  lossbwd_fused   forward and backward down to mean.grad, value.grad and log_std.grad: ppo_loss_kernel, ppo_loss_grad_kernel
  lossbwd_torch   the same through torch's autograd on the same views
For every fused route also the launches alone (the prepared C call between the events, no Python in front of it) and the algorithmic
bytes over that time as a share of the HBM peak (8 TB/s): per sample (2 A + 1) elements for the log-probability, (2 A + 4) elements and
the flag byte for the forward, the same again and (A + 1) elements written for the backward.
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails; the lossbwd pair is measured twice to show the spread between processes. In a process: 3 warm-ups, then the median of 10,
device events around one call.
usage: tools/ppo_loss_cost.py [--json FILE] [--B N] [--K N]"""
import argparse
import ctypes
import json
import math
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

ROUTES = ("logp_fused", "logp_torch", "loss_fused", "loss_torch", "lossbwd_fused", "lossbwd_torch")
GAMMA, LAM, CLIP_EPS, VF, ENT = 0.99, 0.95, 0.2, 0.5, 0.01
HBM_PEAK = 8.0e12  # bytes per second
NET = "16"


def one(route, name, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import MLPPolicy, _native

    assert torch.cuda.is_available(), "ppo_loss_cost.py measures on a HIP device"
    env, state, reset_state, W, b, widths, steps = make(name, B, NETS[NET])
    dt, dev = env.dtype, env.device
    A = widths[-1]
    policy = MLPPolicy(W, b, "tanh", device=dev, dtype=dt)
    noise = env.new_actions_buffer(K)
    noise.normal_(0.0, 0.1)
    ro = env.vmap_rollout_episodes(state, policy, K, env.tau, reset_state, noise=noise, max_episode_steps=MAX_EPISODE_STEPS, episode_steps=steps)
    log_std = torch.full((A,), math.log(0.1), dtype=dt, device=dev)
    with torch.no_grad():
        mean_old = env.vmap_policy_eval(policy, ro.observations, n_rows=K)  # [B, K, A] over [K][A][B]
        sample = noise + mean_old
        logp_old = env.vmap_gaussian_logp(mean_old, sample, log_std)
        value = torch.empty((K + 1, B), dtype=dt, device=dev).normal_().t()  # lane-major like the rollout's rows
        adv, ret = env.vmap_gae(ro.reward, value, GAMMA, LAM, terminated=ro.terminated, reset=ro.reset)
        mean = torch.empty((K, A, B), dtype=dt, device=dev).normal_(0.0, 0.02).permute(2, 0, 1).add_(mean_old)  # a changed policy
        value = value[:, :K]
    reset, mask = ro.reset, (~ro.reset).to(dt)
    elem = mean.element_size()
    samples = B * K
    r = dict(route=route, env=name, A=A, B=B, K=K, reset_share=float(reset.float().mean()))

    def torch_logp(m, ls):
        return (-0.5 * ((sample - m) * torch.exp(-ls)) ** 2).sum(dim=-1) - ls.sum() - 0.5 * A * math.log(2.0 * math.pi)

    def torch_loss(m, v, ls):
        ratio = torch.exp(torch_logp(m, ls) - logp_old)
        surrogate = torch.minimum(ratio * adv, torch.clamp(ratio, 1.0 - CLIP_EPS, 1.0 + CLIP_EPS) * adv)
        n = mask.sum().clamp(min=1.0)
        entropy = ls.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
        loss = -(surrogate * mask).sum() / n + VF * 0.5 * (((v - ret) ** 2) * mask).sum() / n - ENT * entropy
        with torch.no_grad():
            kl = (((ratio - 1.0) - torch.log(ratio)) * mask).sum() / n
            clipped = (((ratio < 1.0 - CLIP_EPS) | (ratio > 1.0 + CLIP_EPS)).to(dt) * mask).sum() / n
        return loss, kl, clipped

    kernel = None
    if route == "logp_fused":
        with torch.no_grad():
            ms = event_ms(lambda: env.vmap_gaussian_logp(mean_old, sample, log_std))
        r["launch"] = _native.last_launch()
        _, inv_std, const = env._ppo_consts(log_std, A)
        out = torch.empty((K, B), dtype=dt, device=dev)
        call = _native.GaussianLogp(mean_old.data_ptr(), sample.data_ptr(), inv_std.data_ptr(), const.data_ptr(), A, out.data_ptr())
        kernel = lambda: _native._launch("excenv_gaussian_logp", out, "cost", _native.dtype_id(dt), B, K, ctypes.byref(call))
        nbytes = samples * (2 * A + 1) * elem
    elif route == "logp_torch":
        with torch.no_grad():
            ms = event_ms(lambda: torch_logp(mean_old, log_std))
        r["launch"] = "elementwise torch"
    elif route in ("loss_fused", "lossbwd_fused"):
        kw = dict(value=value, returns=ret, reset=reset, clip_eps=CLIP_EPS, vf_coef=VF, ent_coef=ENT)
        ls, _, _ = env._ppo_consts(log_std, A)
        _, inv_std, const = env._ppo_consts(log_std, A)
        rows = dict(shape=(B, K, A), mean=mean, sample=sample, inv_std=inv_std, const=const, log_std=ls, clip_eps=CLIP_EPS, max_groups=0,
                    logp_old=logp_old, advantage=adv, value=value, returns=ret, reset=reset, adv_norm=None)
        call = env._ppo_record(rows)
        stats = torch.empty(_native.PPO_STATS + A, dtype=torch.float64, device=dev)
        nb = _native.lib().excenv_ppo_loss_workspace_bytes(B, K, 0)
        work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        call.stats, call.workspace, call.workspace_bytes = stats.data_ptr(), work.data_ptr(), nb
        forward = lambda: _native._launch("excenv_ppo_loss", stats, "cost", _native.dtype_id(dt), B, K, ctypes.byref(call))
        nbytes = samples * ((2 * A + 4) * elem + 1)
        if route == "loss_fused":
            with torch.no_grad():
                ms = event_ms(lambda: env.vmap_ppo_loss(mean, sample, log_std, logp_old, adv, **kw))
            r["launch"] = _native.last_launch() + " + ppo_loss_reduce_kernel"
            kernel = forward
        else:
            m, v, ls_g = mean.detach().requires_grad_(), value.detach().requires_grad_(), log_std.clone().requires_grad_()
            kw["value"] = v

            def both():
                m.grad = v.grad = ls_g.grad = None
                env.vmap_ppo_loss(m, sample, ls_g, logp_old, adv, **kw).loss.backward()

            ms = event_ms(both)
            r["launch"] = "ppo_loss_kernel + ppo_loss_reduce_kernel + ppo_loss_grad_kernel"
            scale = torch.ones(2, dtype=dt, device=dev)
            gm, gv = torch.empty((K, A, B), dtype=dt, device=dev), torch.empty((K, B), dtype=dt, device=dev)
            call.grad_scale, call.grad_mean, call.grad_value = scale.data_ptr(), gm.data_ptr(), gv.data_ptr()

            def kernel():
                forward()
                _native._launch("excenv_ppo_loss_grad", scale, "cost", _native.dtype_id(dt), B, K, ctypes.byref(call))

            nbytes = 2 * nbytes + samples * (A + 1) * elem
    elif route == "loss_torch":
        with torch.no_grad():
            ms = event_ms(lambda: torch_loss(mean, value, log_std))
        r["launch"] = "elementwise torch"
    else:
        m, v, ls_g = mean.detach().requires_grad_(), value.detach().requires_grad_(), log_std.clone().requires_grad_()

        def both():
            m.grad = v.grad = ls_g.grad = None
            torch_loss(m, v, ls_g)[0].backward()

        ms = event_ms(both)
        r["launch"] = "elementwise torch and its autograd"
    med = statistics.median(ms)
    r.update(ms_median=med, ms_min=min(ms), ms_max=max(ms), ns_per_sample=med * 1e6 / samples)
    if kernel is not None:
        km = event_ms(kernel)
        kmed = statistics.median(km)
        r.update(kernel_ms_median=kmed, kernel_ms_min=min(km), kernel_ms_max=max(km), algorithmic_bytes=nbytes,
                 hbm_share=nbytes / (kmed * 1e-3) / HBM_PEAK)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--B", type=int, default=1 << 15)
    ap.add_argument("--K", type=int, default=1000, help="action rows")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=4, metavar=("ROUTE", "ENV", "B", "K"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], int(a.one[2]), int(a.one[3]))))
        return 0
    jobs = [(route, name, 0) for name in ("pendulum", "pmsm") for route in ROUTES]
    jobs += [(route, name, 1) for name in ("pendulum", "pmsm") for route in ("lossbwd_fused", "lossbwd_torch")]  # the pair once more
    results = []
    for route, name, rep in jobs:  # one after the other, each under its own time limit; the first failure ends the session
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", route, name, str(a.B), str(a.K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} B={a.B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        r["repeat"] = rep
        results.append(r)
        tail = f"  launches alone {r['kernel_ms_median']:.3f} ms, {100 * r['hbm_share']:.1f} % of the HBM peak" if "hbm_share" in r else ""
        print(f"{name:9s} A={r['A']} B={a.B:8d} K={a.K:5d} {route:14s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})"
              f"{tail}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
