#!/usr/bin/env python3
"""What the LQR backward pass costs on the Jacobians of a stored trajectory: cart-pole (S, A) = (4, 1) and PMSM (7, 2),
Euler, fp32, B = 4096 and 2^15 environments, N = 100 rows: a `vmap_sim_ahead` trajectory under "step" semantics, `vmap_linearize_ahead`
on it, then on the two views it returned, read in place:
  fused          `vmap_lqr(A, Bu, Q, R)`: ONE launch of riccati_kernel; also the prepared C call alone between the events, and the
                 algorithmic bytes of the call (excenv_lqr_backward_bytes per environment and row, plus the row-0 outputs) over that
                 time as a share of the HBM peak (8 TB/s)
  torch_views    the same recursion in torch on the same views: a loop over the N rows of batched matmul with the closed-form 1 x 1 /
                 2 x 2 solve and the update P = Qxx + Qux^T K (what the recursion reduces to without regularisation): no torch.linalg
  torch_copied   that loop after ONE copy of the views into contiguous [N][B][S][S + A] memory (the copy is inside the timed call)
The torch routes also report the torch operations one call dispatches that compute something (views excluded), counted once outside
the timed calls: each is at least one launch. The gains of the three routes are compared (largest relative difference).
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-ups, then the median of 10, device events around one call.
usage: tools/lqr_cost.py [--json FILE] [--N N]"""
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

from policy_cost import event_ms  # noqa: E402

ROUTES = ("fused", "torch_views", "torch_copied")
ENVS = ("cartpole", "pmsm")
BATCHES = (4096, 1 << 15)
HBM_PEAK = 8.0e12  # bytes per second
VIEW_OPS = ("view", "select", "slice", "transpose", "permute", "expand", "unsqueeze", "squeeze", "alias", "detach", "as_strided", "t.default",
            "reshape", "unsafe_view", "unbind", "split")


def linearised(name, B, N):
    """-> (env, A [B, N, S, S], Bu [B, N, S, action_dim]): the views of `vmap_linearize_ahead` on a seeded trajectory"""
    import torch
    from exciting_environments_amd import EnvironmentRegistry

    reg = {"cartpole": EnvironmentRegistry.CART_POLE, "pmsm": EnvironmentRegistry.PMSM}[name]
    env = reg.make(batch_size=B, dtype=torch.float32, device="cuda:0")
    env.sim_ahead_semantics = "step"
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    _, state = env.vmap_reset()
    if name == "pmsm":  # stable-region speeds
        state.physical_state.omega_el = torch.rand(B, generator=gen, device="cuda:0") * 600.0
        state.physical_state.epsilon = (torch.rand(B, generator=gen, device="cuda:0") - 0.5) * 6.2
    actions = env.new_actions_buffer(N)
    actions.copy_((torch.rand((B, N, env.action_dim), generator=gen, device="cuda:0") - 0.5) * 0.4)
    _, states, _ = env.vmap_sim_ahead(state, actions, env.tau, env.tau)
    A, Bu = env.vmap_linearize_ahead(states, actions, env.tau, env.tau)
    return env, A, Bu


def torch_lqr(A, Bu, Q, R, copied):
    """The recursion in torch -> gain [N, B, action_dim, S]"""
    import torch

    B, N, S, Na = Bu.shape
    if copied:
        Fs, Gs = A.permute(1, 0, 2, 3).contiguous(), Bu.permute(1, 0, 2, 3).contiguous()
    else:
        Fs, Gs = A.permute(1, 0, 2, 3), Bu.permute(1, 0, 2, 3)
    gains = torch.empty((N, B, Na, S), dtype=A.dtype, device=A.device)
    P = Q.expand(B, S, S)
    for n in range(N - 1, -1, -1):
        F, G = Fs[n], Gs[n]
        Ft, Gt = F.transpose(1, 2), G.transpose(1, 2)
        W = torch.matmul(P, F)
        Qux = torch.matmul(Gt, W)
        Quu = R + torch.matmul(Gt, torch.matmul(P, G))
        if Na == 1:
            K = -Qux / Quu
        else:
            a, b, d = Quu[:, 0, 0], Quu[:, 0, 1], Quu[:, 1, 1]
            det = a * d - b * b
            x0 = (d[:, None] * Qux[:, 0] - b[:, None] * Qux[:, 1]) / det[:, None]
            x1 = (a[:, None] * Qux[:, 1] - b[:, None] * Qux[:, 0]) / det[:, None]
            K = -torch.stack((x0, x1), dim=1)
        P = Q + torch.matmul(Ft, W) + torch.matmul(Qux.transpose(1, 2), K)
        gains[n] = K
    return gains


def count_ops(fn):
    """The aten operations one call of fn dispatches, views excluded"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not any(v in str(func) for v in VIEW_OPS):
                Count.n += 1
            return func(*args, **(kwargs or {}))

    with Count():
        fn()
    return Count.n


def one(route, name, B, N):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import _native

    assert torch.cuda.is_available(), "lqr_cost.py measures on a HIP device"
    env, A, Bu = linearised(name, B, N)
    dt, dev = env.dtype, env.device
    S, Na = env.physical_state_dim, env.action_dim
    Q = torch.eye(S, dtype=dt, device=dev)
    R = torch.eye(Na, dtype=dt, device=dev)
    r = dict(route=route, env=name, B=B, N=N, S=S, A=Na)
    ref = env.vmap_lqr(A, Bu, Q, R)
    assert env.last_lqr_in_place
    r["n_bad"] = int(ref.n_bad.sum())
    with torch.no_grad():
        if route == "fused":
            ms = event_ms(lambda: env.vmap_lqr(A, Bu, Q, R))
            r["launch"], r["launches"] = env.last_lqr_launch, 1
            out = [torch.empty(s, dtype=dt, device=dev) for s in ((N, Na, S, B), (N, Na, B), (S, S, B), (S, B), (2, B))]
            n_bad = torch.empty(B, dtype=torch.int32, device=dev)
            call = _native.Lqr(S, Na, A.data_ptr(), S * (S + Na) * B, Q.data_ptr(), None, R.data_ptr(), None, None, 0.0, 1,
                               *[t.data_ptr() for t in out], n_bad.data_ptr())
            km = event_ms(lambda: _native._launch("excenv_lqr_backward", n_bad, "cost", _native.dtype_id(dt), B, N, ctypes.byref(call)))
            elem = A.element_size()
            nbytes = B * (N * _native.lib().excenv_lqr_backward_bytes(_native.dtype_id(dt), S, Na, 0, 0, 0, 1, 1) + (S * S + S + 2) * elem + 4)
            kmed = statistics.median(km)
            r.update(kernel_ms_median=kmed, kernel_ms_min=min(km), kernel_ms_max=max(km), algorithmic_bytes=nbytes,
                     hbm_share=nbytes / (kmed * 1e-3) / HBM_PEAK, us_per_row=kmed * 1e3 / N)
            r["gain_rel_diff"] = 0.0
        else:
            f = lambda: torch_lqr(A, Bu, Q, R, route == "torch_copied")
            ms = event_ms(f)
            r["launch"] = "torch: batched matmul and the closed-form solve, a loop over the rows"
            r["launches"] = count_ops(f)
            g = f().permute(1, 0, 2, 3)
            r["gain_rel_diff"] = float((g - ref.gain).abs().max() / ref.gain.abs().max())
    med = statistics.median(ms)
    r.update(ms_median=med, ms_min=min(ms), ms_max=max(ms))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--N", type=int, default=100, help="rows")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=4, metavar=("ROUTE", "ENV", "B", "N"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], int(a.one[2]), int(a.one[3]))))
        return 0
    results = []
    for name in ENVS:
        for B in BATCHES:
            for route in ROUTES:  # one after the other, each under its own time limit; the first failure ends the session
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", route, name, str(B), str(a.N)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(f"{route} {name} B={B}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                    if a.json and results:
                        json.dump(dict(complete=False, results=results), open(a.json, "w"), indent=1)
                    return 1
                r = json.loads(line[0][7:])
                results.append(r)
                tail = (f"  launch alone {r['kernel_ms_median']:.3f} ms = {r['us_per_row']:.2f} us a row, {100 * r['hbm_share']:.1f} % of the HBM peak"
                        if "hbm_share" in r else f"  gains differ by {r['gain_rel_diff']:.2e} (relative)")
                print(f"{name:9s} B={B:6d} N={a.N:4d} {route:13s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}) "
                      f"{r['launches']:5d} launches{tail}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
