#!/usr/bin/env python3
"""What a batched linearisation costs next to the route a user had before it, in one process and on the same state: PMSM and
pendulum, RK4 and Euler, fp32, at B = 2^15 and B = 2^20.
  linearize      one `vmap_linearize(state, action, new_state)`: one launch of step_jac_kernel
  one_hot_route  S calls of `vmap_step_vjp(state, action, new_state, grad_state=e_r)` with one-hot cotangents, then the torch.stack of
                 their results into A [B, S, S] and Bu [B, S, A]: S launches of step_vjp_kernel plus the stacking
and for a stored trajectory of N = 32 steps ("step" semantics)
  linearize_ahead  one `vmap_linearize_ahead(states, actions, tau, tau)`
  single_calls     N calls of `vmap_linearize` on the trajectory's rows
The small size is timed with the host clock around `--inner` calls ending in a device synchronise (what a caller waits for: launch
overheads included), the large size with device events; each figure is the median of `--reps` windows, the two routes of a pair
alternate, and every pair is timed twice (the spread). Both routes are checked against each other before they are timed.
The linearize launch's algorithmic bytes come from excenv_step_jacobian_bytes; its fraction of the 8 TB/s HBM peak is reported at
the large size.
usage: tools/step_jac_cost.py [--small B] [--large B] [--rows N] [--reps N] [--inner N] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK = 8.0e12  # bytes / s
DEV = "cuda:0"


def make(reg, name, solver, B):
    import exciting_environments_amd as ex

    env = reg.make(batch_size=B, dtype=torch.float32, device=DEV, solver={"euler": ex.Euler(), "rk4": ex.RK4()}[solver])
    env.sim_ahead_semantics = "step"
    _, state = env.vmap_reset()
    if name == "pmsm":
        state.physical_state.omega_el = torch.rand(B, device=DEV) * 600
        state.physical_state.epsilon = (torch.rand(B, device=DEV) - 0.5) * 6
    return env, state


def window_us(fn, inner, device):
    """the time of one fn() in us over a window of `inner` calls: device events, or the host clock ending in a synchronise"""
    if device:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        return float(t0.elapsed_time(t1)) / inner * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def pair_us(fa, fb, reps, inner, device, warm=3):
    """medians over `reps` alternating windows of fa and fb, the whole thing twice -> ([a, a'], [b, b'])"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    out_a, out_b = [], []
    for _ in range(2):
        a, b = [], []
        for _ in range(reps):
            a.append(window_us(fa, inner, device))
            b.append(window_us(fb, inner, device))
        out_a.append(round(statistics.median(a), 2))
        out_b.append(round(statistics.median(b), 2))
    return out_a, out_b


def rel_diff(x, y):
    return float((x - y).abs().max() / y.abs().max())


def measure(name, reg, solver, B, rows, reps, inner, device):
    from exciting_environments_amd import _native

    env, state = make(reg, name, solver, B)
    S, A = env.physical_state_dim, env.action_dim
    action = (torch.rand(B, A, device=DEV) - 0.5) * 1.5
    _, new_state = env.vmap_step(state, action)
    new_state = env.State(env.PhysicalState(*[getattr(new_state.physical_state, n).clone() for n in env.STATE_FIELDS]),
                          new_state.PRNGKey, new_state.additions, new_state.reference)  # not a pool slot a later step reuses
    one = torch.ones(B, device=DEV)
    hot = [[one if j == r else None for j in range(S)] for r in range(S)]

    def linearize():
        return env.vmap_linearize(state, action, new_state)

    def one_hot_route():
        ga, gs = zip(*[env.vmap_step_vjp(state, action, new_state, grad_state=hot[r]) for r in range(S)])
        return (torch.stack([torch.stack([getattr(g, n) for n in env.STATE_FIELDS], dim=-1) for g in gs], dim=1),
                torch.stack(ga, dim=1))

    (a0, b0), (a1, b1) = linearize(), one_hot_route()
    torch.cuda.synchronize()
    launch = env.last_linearize_launch
    diff = max(rel_diff(a0, a1), rel_diff(b0, b1))
    lin, hotr = pair_us(linearize, one_hot_route, reps, inner, device)
    nbytes = _native.step_jacobian_bytes(env.ENV_ID, env.dtype, "state")
    out = {"workload": f"{name} {solver} fp32", "B": B, "clock": "device events" if device else "host, synchronised", "launch": launch,
           "linearize_us": lin, "one_hot_route_us": hotr, "calls_replaced": S, "rel_diff": diff,
           "one_hot_over_linearize": round(min(hotr) / min(lin), 2), "bytes_per_instance": nbytes}
    if device:
        out["fraction_of_peak"] = round(nbytes * B / (min(lin) * 1e-6) / PEAK, 4)
    # a stored trajectory
    tau = env.tau
    actions = env.new_actions_buffer(rows)
    actions.copy_((torch.rand(B, rows, A, device=DEV) - 0.5) * 1.5)
    _, states, _ = env.vmap_sim_ahead(state, actions, tau, tau)
    traj = [getattr(states.physical_state, n).clone() for n in env.STATE_FIELDS]  # clone keeps the lane-major strides

    def ahead():
        return env.vmap_linearize_ahead(traj, actions, tau, tau)

    def single_calls():
        return [env.vmap_linearize([t[:, n] for t in traj], actions[:, n], [t[:, n + 1] for t in traj]) for n in range(rows)]

    (ja, jb), singles = ahead(), single_calls()
    torch.cuda.synchronize()
    adiff = max(max(rel_diff(ja[:, n], singles[n][0]), rel_diff(jb[:, n], singles[n][1])) for n in range(rows))
    del singles
    inner_t = max(1, inner // rows)
    ah, sc = pair_us(ahead, single_calls, reps, inner_t, device)
    out["trajectory"] = {"rows": rows, "linearize_ahead_us": ah, "single_calls_us": sc, "rel_diff": adiff,
                         "single_over_ahead": round(min(sc) / min(ah), 2)}
    if device:
        out["trajectory"]["fraction_of_peak"] = round(nbytes * B * rows / (min(ah) * 1e-6) / PEAK, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=1 << 15)
    ap.add_argument("--large", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "step_jac_cost.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU: no device, no figures"
    from exciting_environments_amd import EnvironmentRegistry

    res = []
    for name, reg in (("pmsm", EnvironmentRegistry.PMSM), ("pendulum", EnvironmentRegistry.PENDULUM)):
        for solver in ("rk4", "euler"):
            for B, device in ((a.small, False), (a.large, True)):
                r = measure(name, reg, solver, B, a.rows, a.reps, a.inner if not device else max(4, a.inner // 4), device)
                print(json.dumps(r), flush=True)
                res.append(r)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
