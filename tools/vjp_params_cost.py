#!/usr/bin/env python3
"""What the parameter gradients cost: the plain backward launch (excenv_sim_ahead_vjp) against the PGRAD backward launch
(excenv_sim_ahead_vjp_params, all differentiable leaves requested) over the same buffers in one process — PMSM Euler fp32 and
pendulum Euler fp32 at B = 2^20, K = 100 (options below), all three cotangent groups present, median of the timed launches after
warm-up. Both launches move the same bytes (the PGRAD one stores P x [B] once per trajectory on top), so whatever the ratio
exceeds 1 by is arithmetic, registers or the fall-back to one environment per lane (PMSM). The batch sum (excenv_param_grad_sum)
is timed separately. Like tools/vjp_cost.py the timings include the Python call and the allocation of the outputs.
usage: tools/vjp_params_cost.py [--batch B] [--steps K] [--reps N] [--json FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "exciting-environments_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from vjp_cost import timed  # noqa: E402


def workload(name, reg, B, K, reps):
    from exciting_environments_amd import _native

    env = reg.make(batch_size=B, dtype=torch.float32, device="cuda:0")
    _, state = env.vmap_reset()
    if name == "pmsm":
        state.physical_state.omega_el = torch.rand(B, device="cuda:0") * 600
        state.physical_state.epsilon = (torch.rand(B, device="cuda:0") - 0.5) * 6
    actions = env.new_actions_buffer(K)
    actions.copy_((torch.rand(B, K, env.action_dim, device="cuda:0") - 0.5) * 1.5)
    tau = env.tau
    obs, states, last = env.vmap_sim_ahead(state, actions, tau, tau)
    g_obs = torch.empty_like(obs).normal_()  # empty_like keeps the lane-major strides
    g_states = [torch.empty_like(getattr(states.physical_state, n)).normal_() for n in env.STATE_FIELDS]
    g_last = [torch.randn(B, device="cuda:0") for _ in env.STATE_FIELDS]
    out = {"workload": f"{name} euler fp32", "B": B, "K": K}
    plain = timed(lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, g_obs, g_states, g_last), reps)
    out["backward_plain"] = {"ms": round(plain, 4), "launch": _native.last_launch()}
    pgrad = timed(lambda: env.vmap_sim_ahead_vjp(states, actions, tau, tau, g_obs, g_states, g_last, param_grads="per_env"), reps)
    out["backward_pgrad"] = {"ms": round(pgrad, 4), "launch": _native.last_launch()}
    out["ratio"] = round(pgrad / plain, 3)
    gp = env.vmap_sim_ahead_vjp(states, actions, tau, tau, g_obs, g_states, g_last, param_grads="per_env")[2]
    per_env = [getattr(gp, n) for n in env.PARAM_FIELDS if getattr(gp, n) is not None]
    out["param_grad_sum"] = {"ms": round(timed(lambda: env._param_grad_sum(per_env), reps), 4), "leaves": len(per_env)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from exciting_environments_amd import EnvironmentRegistry

    res = []
    for name, reg in (("pmsm", EnvironmentRegistry.PMSM), ("pendulum", EnvironmentRegistry.PENDULUM)):
        r = workload(name, reg, a.batch, a.steps, a.reps)
        print(json.dumps(r))
        res.append(r)
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
