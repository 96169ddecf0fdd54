#!/usr/bin/env python3
"""What the rollout statistics cost on the rows of an episode rollout: pendulum, Euler, fp32, a tanh network with one
hidden layer of 16, `vmap_rollout_episodes` at B = 2^15 with K = 1000 action rows (the rollout of tools/episode_cost.py). On its views and
on `vmap_gae`'s advantages, read in place:
  advnorm_fused    `vmap_advantage_norm(adv, ro.reset)`: row_moments_kernel and its reduction, then the scalar ops
  advnorm_torch    the same two numbers without a synchronisation: torch.where on the mask, then the count, the sum and the sum of squares
  advnorm_index    `adv[~reset].mean()` / `.std()`: the boolean index with its nonzero and host synchronisation
  obsmom_fused     `vmap_row_moments(ro.observations[:, :K], mask=ro.reset)`: the OW observation columns in one call
  obsmom_torch     torch.where on the mask broadcast over the columns, then the sums over (batch, rows)
  episodes_fused   `vmap_episode_stats(ro.reward, ro.reset, episode_steps=steps)`: episode_stats_kernel and its reduction
  episodes_torch   the same statistics as a segmented scan in torch: cumsum of the kept rewards, the row of the last reset by cummax, gathers
  columns_C        (C = 1, 2, 4, 8, 16) the launches of excenv_row_moments alone on a random [K][C][B] array under the rollout's mask: how
                   the share of the HBM peak moves with the bytes a lane has in flight (a pass of the kernel holds 1, 2 or 4 columns)
For every fused route also the launches alone (the prepared C call between the events, no Python in front of it) and the algorithmic
bytes over that time as a share of the HBM peak (8 TB/s): per sample C elements and the mask byte for the moments, one element and the
flag byte for the episode scan.
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-ups, then the median of 10, device events around one call.
usage: tools/rollout_stats_cost.py [--json FILE] [--B N] [--K N]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from episode_cost import MAX_EPISODE_STEPS, make  # noqa: E402  (the same environment, network and rollout)
from policy_cost import NETS, event_ms  # noqa: E402

ROUTES = ("advnorm_fused", "advnorm_torch", "advnorm_index", "obsmom_fused", "obsmom_torch", "episodes_fused", "episodes_torch",
          "columns_1", "columns_2", "columns_4", "columns_8", "columns_16")
GAMMA, LAM, EPS = 0.99, 0.95, 1e-8
HBM_PEAK = 8.0e12  # bytes per second
NET = "16"


def one(route, name, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import MLPPolicy, _native

    assert torch.cuda.is_available(), "rollout_stats_cost.py measures on a HIP device"
    env, state, reset_state, W, b, widths, steps = make(name, B, NETS[NET])
    dt, dev = env.dtype, env.device
    for st in (state, reset_state):  # a finite reference for the controlled angle (a reset state's is NaN), so that the rewards are numbers
        st.reference.theta = torch.zeros(B, dtype=dt, device=dev)
    policy = MLPPolicy(W, b, "tanh", device=dev, dtype=dt)
    noise = env.new_actions_buffer(K)
    noise.normal_(0.0, 0.1)
    ro = env.vmap_rollout_episodes(state, policy, K, env.tau, reset_state, noise=noise, max_episode_steps=MAX_EPISODE_STEPS, episode_steps=steps)
    with torch.no_grad():
        value = torch.empty((K + 1, B), dtype=dt, device=dev).normal_().t()  # lane-major like the rollout's rows
        adv, _ = env.vmap_gae(ro.reward, value, GAMMA, LAM, terminated=ro.terminated, reset=ro.reset)
    reset, reward = ro.reset, ro.reward
    obs = ro.observations[:, :K]  # [B, K, OW] over [K + 1][OW][B]
    OW = obs.shape[2]
    elem = adv.element_size()
    samples = B * K
    r = dict(route=route, env=name, B=B, K=K, OW=OW, reset_share=float(reset.float().mean()))
    zero = torch.zeros((), dtype=dt, device=dev)
    kernel = None

    def moments_call(x, C):
        stats = torch.empty(1 + 2 * C, dtype=torch.float64, device=dev)
        nb = _native.lib().excenv_row_moments_workspace_bytes(B, K, C, 0)
        work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        call = _native.RowMoments(x.data_ptr(), reset.data_ptr(), None, C, 0, stats.data_ptr(), work.data_ptr(), nb)
        keep = (stats, work, call)
        return lambda: (keep, _native._launch("excenv_row_moments", stats, "cost", _native.dtype_id(dt), B, K, ctypes.byref(call)))[1]

    with torch.no_grad():
        if route == "advnorm_fused":
            assert tuple(adv.stride()) == (1, B) and tuple(reset.stride()) == (1, B)
            ms = event_ms(lambda: env.vmap_advantage_norm(adv, reset, eps=EPS))
            r["launch"] = _native.last_launch() + " + rollout_stats_reduce_kernel"
            r["value"] = [float(v) for v in env.vmap_advantage_norm(adv, reset, eps=EPS)]
            kernel, nbytes = moments_call(adv, 1), samples * (elem + 1)
        elif route == "advnorm_torch":
            def f():
                a = torch.where(reset, zero, adv)
                n = (~reset).sum().to(torch.float64)
                s1, s2 = a.sum(dtype=torch.float64), (a * a).sum(dtype=torch.float64)
                n1 = n.clamp(min=1.0)
                return s1 / n1, 1.0 / (torch.sqrt(((s2 - s1 * s1 / n1) / (n - 1.0).clamp(min=1.0)).clamp(min=0.0)) + EPS)
            ms = event_ms(f)
            r["launch"] = "elementwise torch, no synchronisation"
            r["value"] = [float(v) for v in f()]
        elif route == "advnorm_index":
            def f():
                a = adv[~reset]
                return a.mean(), 1.0 / (a.std() + EPS)
            ms = event_ms(f)
            r["launch"] = "boolean index (nonzero, host synchronisation)"
            r["value"] = [float(v) for v in f()]
        elif route == "obsmom_fused":
            assert tuple(obs.stride()) == (1, OW * B, B)
            ms = event_ms(lambda: env.vmap_row_moments(obs, mask=reset))
            r["launch"] = _native.last_launch() + " + rollout_stats_reduce_kernel"
            r["value"] = env.vmap_row_moments(obs, mask=reset).mean.tolist()
            kernel, nbytes = moments_call(obs, OW), samples * (OW * elem + 1)
        elif route == "obsmom_torch":
            def f():
                o = torch.where(reset.unsqueeze(-1), zero, obs)
                n1 = (~reset).sum().to(torch.float64).clamp(min=1.0)
                s1, s2 = o.sum(dim=(0, 1), dtype=torch.float64), (o * o).sum(dim=(0, 1), dtype=torch.float64)
                return s1 / n1, ((s2 - s1 * s1 / n1) / n1).clamp(min=0.0)
            ms = event_ms(f)
            r["launch"] = "elementwise torch, no synchronisation"
            r["value"] = f()[0].tolist()
        elif route.startswith("columns_"):
            C = int(route.split("_")[1])
            x = torch.empty((K, C, B), dtype=dt, device=dev).normal_()
            kernel, nbytes = moments_call(x, C), samples * (C * elem + 1)
            ms = event_ms(kernel)
            r["launch"] = "row_moments_kernel + rollout_stats_reduce_kernel (the C call alone)"
            r["value"] = [float(C)]
        elif route == "episodes_fused":
            ms = event_ms(lambda: env.vmap_episode_stats(reward, reset, episode_steps=steps))
            r["launch"] = _native.last_launch() + " + rollout_stats_reduce_kernel"
            e = env.vmap_episode_stats(reward, reset, episode_steps=steps)
            r["value"] = [float(v) for v in e[:6]]
            stats = torch.empty(_native.EPISODE_STATS, dtype=torch.float64, device=dev)
            nb = _native.lib().excenv_episode_stats_workspace_bytes(B)
            work = torch.empty(nb // 8, dtype=torch.float64, device=dev)
            ret_out, steps_out = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            call = _native.EpisodeStats(reward.data_ptr(), reset.data_ptr(), None, steps.data_ptr(), None, ret_out.data_ptr(), steps_out.data_ptr(),
                                        stats.data_ptr(), work.data_ptr(), nb)
            kernel = lambda: _native._launch("excenv_episode_stats", stats, "cost", _native.dtype_id(dt), B, K, ctypes.byref(call))
            nbytes = samples * (elem + 1) + B * 16
        else:
            rows = torch.arange(K, device=dev).unsqueeze(0)

            def f():
                kept = torch.where(reset, zero, reward).to(torch.float64)
                c = kept.cumsum(dim=1)
                last = torch.where(reset, rows, -1).cummax(dim=1).values                # the last reset at or before row n
                prev = torch.cat((torch.full_like(last[:, :1], -1), last[:, :-1]), dim=1)  # ... strictly before row n
                base = torch.where(prev >= 0, c.gather(1, prev.clamp(min=0)), torch.zeros((), dtype=torch.float64, device=dev))
                length = torch.where(prev >= 0, rows - prev - 1, rows + steps.unsqueeze(1).to(torch.int64))
                emit = reset & (length > 0)
                ret = torch.where(emit, c - base, torch.zeros((), dtype=torch.float64, device=dev))
                n = emit.sum().to(torch.float64)
                n1 = n.clamp(min=1.0)
                sr, srr = ret.sum(), (ret * ret).sum()
                inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
                return (n, sr / n1, torch.sqrt(((srr - sr * sr / n1) / n1).clamp(min=0.0)), torch.where(emit, length, 0).sum().to(torch.float64) / n1,
                        torch.where(emit, ret, inf).min(), torch.where(emit, ret, -inf).max())
            ms = event_ms(f)
            r["launch"] = "segmented scan in torch (cumsum, cummax, gather), no synchronisation"
            r["value"] = [float(v) for v in f()]
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
    results = []
    for route in ROUTES:  # one after the other, each under its own time limit; the first failure ends the session
        name = "pendulum"
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", route, name, str(a.B), str(a.K)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{route} {name} B={a.B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            if a.json and results:
                json.dump(dict(complete=False, results=results), open(a.json, "w"), indent=1)
            return 1
        r = json.loads(line[0][7:])
        results.append(r)
        tail = f"  launches alone {r['kernel_ms_median']:.3f} ms, {100 * r['hbm_share']:.1f} % of the HBM peak" if "hbm_share" in r else ""
        print(f"{name:9s} B={a.B:8d} K={a.K:5d} {route:15s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}){tail}   "
              f"[{r['launch']}]  -> {['%.6g' % v for v in r['value']]}", flush=True)
    if a.json:
        json.dump(dict(complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
