#!/usr/bin/env python3
"""What an episode rollout costs per action row next to the two routes that existed before it: pendulum [theta] and PMSM [i_d, i_q],
Euler, fp32, B = 2^15, K action rows, tanh networks with hidden widths (64, 64) and (16,), max_episode_steps = 200:
  episodes         one `vmap_rollout_episodes` (noise rows read, clip (-1, 1), both end conditions, one reset row; state trajectory,
                   actions, reward, flags, reset and counters written): one launch of sim_episodes_kernel
  policy_then_gym  `vmap_sim_ahead_policy` + `vmap_generate_rew_trunc_term_ahead` on its states: two launches, no resets — the
                   cheapest thing a user could do before
  host_loop        the one route with episode boundaries before: per step the MLP as torch launches (addmm, tanh per hidden layer,
                   add, clamp), one `vmap_gym_step`, and `torch.where` on every state leaf (and on the step counter) for the resets
Every measurement runs in a fresh process under its own `timeout`; the driver starts them one after the other and stops at the first
that fails. In a process: 3 warm-up runs, then the median of 10 timed ones (device events around the launches; the host loop by the
host clock around a window that ends in a device synchronise). No test asserts a time.
usage: tools/episode_cost.py [--json FILE] [--B B] [--K N]"""
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

from policy_cost import DEV, NETS, event_ms, host_ms  # noqa: E402  (the same timing windows as tools/policy_cost.py)

CONTROL = {"pendulum": ["theta"], "pmsm": ["i_d", "i_q"]}
MAX_EPISODE_STEPS = 200
ROUTES = ("episodes", "policy_then_gym", "host_loop")


def make(name, B, hidden):
    import torch
    from exciting_environments_amd import EnvironmentRegistry

    reg = {"pendulum": EnvironmentRegistry.PENDULUM, "pmsm": EnvironmentRegistry.PMSM}[name]
    env = reg.make(batch_size=B, dtype=torch.float32, device=DEV, control_state=CONTROL[name])
    env.sim_ahead_semantics = "step"
    _, state = env.vmap_reset()
    _, reset_state = env.vmap_reset()
    g = torch.Generator(device="cpu").manual_seed(3)
    for s in (state, reset_state):
        if name == "pmsm":
            s.physical_state.omega_el = (torch.rand(B, generator=g) * 600).to(DEV)
            s.physical_state.epsilon = ((torch.rand(B, generator=g) - 0.5) * 6).to(DEV)
        else:
            s.physical_state.theta = ((torch.rand(B, generator=g) - 0.5) * 6).to(DEV)
    widths = (env._obs_dim(),) + tuple(hidden) + (env.action_dim,)
    W = [torch.randn(d, n, generator=g) / n ** 0.5 for n, d in zip(widths[:-1], widths[1:])]
    b = [(torch.rand(d, generator=g) - 0.5) * 0.2 for d in widths[1:]]
    steps = torch.randint(0, MAX_EPISODE_STEPS, (B,), generator=g, dtype=torch.int32).to(DEV)
    return env, state, reset_state, W, b, widths, steps


def one(route, name, net, B, K):
    """One measurement in this (fresh) process -> dict"""
    import torch
    from exciting_environments_amd import MLPPolicy

    assert torch.cuda.is_available(), "episode_cost.py measures on a HIP device"
    env, state, reset_state, W, b, widths, steps = make(name, B, NETS[net])
    tau = env.tau
    extra = {}
    if route in ("episodes", "policy_then_gym"):
        policy = MLPPolicy(W, b, "tanh")
        noise = env.new_actions_buffer(K)
        noise.normal_(0.0, 0.1)
        if route == "episodes":
            fn = lambda: env.vmap_rollout_episodes(state, policy, K, tau, reset_state, noise=noise, max_episode_steps=MAX_EPISODE_STEPS,
                                                   episode_steps=steps)
            ms = event_ms(fn)
            r = fn()
            extra["reset_share"] = float(r.reset.float().mean())
        else:
            def fn():
                _, states, _, actions = env.vmap_sim_ahead_policy(state, policy, K, tau, tau, noise=noise)
                return env.vmap_generate_rew_trunc_term_ahead(states, actions)

            ms = event_ms(fn)
        launch = env.last_policy_launch
    else:  # host_loop
        Wt = [w.t().contiguous().to(DEV) for w in W]
        bd = [v.to(DEV) for v in b]
        noise = (torch.randn(K, B, env.action_dim) * 0.1).to(DEV)
        fields = env.STATE_FIELDS
        rows = [getattr(reset_state.physical_state, f) for f in fields]
        obs0 = env.generate_observation(state, env.env_properties)

        def fn():
            st, ob, t = state, obs0, steps
            end = torch.zeros(B, dtype=torch.bool, device=DEV)
            for k in range(K):
                x = ob
                for l in range(len(Wt) - 1):
                    x = torch.tanh(torch.addmm(bd[l], x, Wt[l]))
                a = torch.clamp(torch.addmm(bd[-1], x, Wt[-1]) + noise[k], -1.0, 1.0)
                ob, _, term, trunc, st = env.vmap_gym_step(st, a)
                # (the flags of the new row end the episode at the next step: the next row of these lanes is the reset row)
                end = term.reshape(-1) | trunc.any(dim=1) | (t + 1 >= MAX_EPISODE_STEPS)
                for f, row in zip(fields, rows):
                    setattr(st.physical_state, f, torch.where(end, row, getattr(st.physical_state, f)))
                t = torch.where(end, 0, t + 1)

        ms = host_ms(fn)
        launch = "vmap_gym_step per step + the MLP and torch.where in torch"
    med = statistics.median(ms)
    return dict(route=route, env=name, net=net, widths=list(widths), B=B, K=K, launch=launch, ms_median=med, ms_min=min(ms), ms_max=max(ms),
                us_per_row=med * 1e3 / K, **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--B", type=int, default=1 << 15)
    ap.add_argument("--K", type=int, default=1000, help="action rows")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per measurement")
    ap.add_argument("--one", nargs=4, metavar=("ROUTE", "ENV", "NET", "B"), help="(internal) one measurement in this process, JSON on stdout")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], a.one[1], a.one[2], int(a.one[3]), a.K)))
        return 0
    results = []
    for name in ("pendulum", "pmsm"):
        for net in NETS:
            for route in ROUTES:  # one after the other, each under its own time limit; the first failure ends the session
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--K", str(a.K), "--one", route, name,
                       net, str(a.B)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(f"{route} {name} {net}: exit status {p.returncode}; stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                    if a.json and results:
                        json.dump(dict(max_episode_steps=MAX_EPISODE_STEPS, complete=False, results=results), open(a.json, "w"), indent=1)
                    return 1
                r = json.loads(line[0][7:])
                results.append(r)
                share = f"  resets {r['reset_share']:.4f} of the rows" if "reset_share" in r else ""
                print(f"{name:9s} B={a.B:7d} {route:16s} net {r['net']:6s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f})  "
                      f"{r['us_per_row']:8.3f} us / row{share}   [{r['launch']}]", flush=True)
    if a.json:
        json.dump(dict(max_episode_steps=MAX_EPISODE_STEPS, complete=True, results=results), open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
