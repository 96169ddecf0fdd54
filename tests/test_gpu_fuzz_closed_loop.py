"""Randomised cross-configuration tests of the closed-loop launches (``-m gpu``): `vmap_sim_ahead_feedback` (sim_feedback_kernel), its
reverse mode `vmap_sim_ahead_feedback_vjp` (feedback_z_rows_kernel, sim_feedback_vjp_kernel, feedback_gain_grad_kernel, the chunked
batch sum of param_sum.hip) and `vmap_sim_ahead_policy` (sim_policy_kernel).

tests/helpers_fuzz_closed_loop.py draws the configurations (its module text lists the axes; tests/test_fuzz_closed_loop_host.py holds
the draws to their input conditions without a GPU). Seeds are fixed: a failure prints the full configuration and reproduces.
EXCENV_FUZZ_SEEDS sets the number of draws per family (default 24), as in tests/test_gpu_fuzz.py.

No tolerance is new. Every check is one of the fixed suites', against the same references:
(a) feedback: tests/test_gpu_feedback.py's check_dynamics (the open-loop kernel on the returned actions, bit for bit), check_policy
    (helpers_feedback.policy_bounds on the returned observation rows) and, in fp64, check_independent (helpers_feedback.
    oracle_closed_loop; 100 x the open-loop distance, floor 1e-12);
(b) reverse: tests/test_gpu_feedback_vjp.py's compare / check against helpers_feedback_vjp.twin_run / twin_grads: 1e-8 in fp64; in fp32
    32 x the forward floor with the environments inside KINK_MARGIN excluded (that file's test 3). One gain set for all: the result is,
    bit for bit, excenv_param_grad_sum of the per-environment launch on the same gains (assert_batch_sum_identity). A sum over the batch
    cannot leave environments out, so in fp32 the per-environment launch is what meets the twin under the exclusion, the sum is tied to
    it by that identity, and the sum itself meets the twin's where no environment is excluded. One draw in four asks for
    per-environment properties or the saturated PMSM and asserts the refusal by name; nothing is launched there;
(c) policy: tests/test_gpu_policy.py's check_dynamics, check_policy (bit for bit through helpers_policy.fma_exact for ReLU and L = 1,
    helpers_policy.policy_bounds for tanh) and, in fp64, check_independent (helpers_policy.oracle_policy_loop).
With K = 0 there is no action row for the open-loop kernel to be handed: the state and the integrator pass through bit for bit and
row 0 is the open-loop launch's row 0.
Every draw prints its configuration and its largest error over bound."""
import numpy as np
import pytest
import torch

import helpers_feedback as hf
import helpers_feedback_vjp as hv
import helpers_fuzz_closed_loop as fz
import helpers_policy as hp
import oracle
from helpers import make_env
from helpers_vjp import KINK_CAP, KINK_MARGIN, obs_floor

pytestmark = pytest.mark.gpu
SEEDS = range(fz.n_seeds())


def _forward_env(cfg, spec):
    """-> (env, spec, float64 oracle properties and what keeps them alive)"""
    tdt = getattr(torch, cfg["dtype"])
    control = cfg["control"] or None
    if cfg["env_name"] == fz.SATURATED:
        env, props, keep, spec = hf.saturated_env(cfg["B"], tdt, cfg["solver"], "cuda", control_state=control)
    else:
        env, _, _, _ = make_env(cfg["env_name"], cfg["B"], tdt, cfg["solver"], spec=spec, control_state=control)
        props, keep = oracle.make_props(cfg["env_name"], spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, cfg["B"])
    env.store_state_trajectory = cfg["store_states"]
    return env, spec, (props, keep)


def _row_zero_only(run, inp, env, z0=None):
    """K = 0: one row, no action; the state (and the integrator) pass through; row 0 is the open-loop launch's"""
    assert run["obs"].shape[1] == 1 and run["actions"].shape[1] == 0
    dev = lambda v: torch.as_tensor(np.asarray(v), dtype=env.dtype, device=env.device)
    for n, v in zip(env.STATE_FIELDS, inp["st"]):
        assert torch.equal(getattr(run["last"].physical_state, n), dev(v)), n
    if run.get("z") is not None:
        assert torch.equal(run["z"], torch.zeros_like(run["z"]) if z0 is None else dev(z0))
    keep = env.sim_ahead_semantics
    env.sim_ahead_semantics = "step"
    try:
        obs, _, _ = env.vmap_sim_ahead(run["state"], run["actions"], run["tau"], run["tau"] * run["sub"])
    finally:
        env.sim_ahead_semantics = keep
    assert torch.equal(obs, run["obs"])


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("i", SEEDS)
def test_random_closed_loop_configuration(i):
    from test_gpu_feedback import check_dynamics, check_independent, check_policy, closed_loop

    cfg, spec = fz.draw("feedback", i)
    print("feedback draw:", fz.describe(cfg))
    model, K, sub = fz.model_of(cfg), cfg["K"], cfg["substeps"]
    env, spec, (props, _keep) = _forward_env(cfg, spec)
    inp = fz.feedback_case(cfg, spec)
    control = cfg["control"] or None
    try:
        run = closed_loop(env, inp, K, sub, spec["tau"], clip=cfg["clip"], control=control, plain_ff=cfg["feedforward"] == "plain")
        assert (run["states"] is None) == (not cfg["store_states"])
        if K > 0:
            check_dynamics(run)
        else:
            _row_zero_only(run, inp, env, inp["z0"])
        check_policy(run, inp, clip=cfg["clip"])
        worst = 0.0
        if cfg["dtype"] == "float64":
            want = hf.oracle_closed_loop(model, cfg["solver"], props, inp, spec["tau"], K=K, sub=sub, clip=cfg["clip"], control=control)
            worst = check_independent(run, inp, props, want, model, cfg["solver"], spec["tau"], f"feedback draw {i}", control=control)
        assert bool(torch.isfinite(run["obs"]).all())
    except AssertionError as e:
        raise AssertionError(f"feedback draw {i}: {fz.describe(cfg)}\n{e}") from e
    print(f"feedback draw {i}: passed; independent loop distance / allowed {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("i", SEEDS)
def test_random_policy_configuration(i):
    from test_gpu_policy import check_bound, check_dynamics, check_exact, check_independent, rollout

    cfg, spec = fz.draw("policy", i)
    print("policy draw:", fz.describe(cfg))
    model, K, sub = fz.model_of(cfg), cfg["K"], cfg["substeps"]
    env, spec, (props, _keep) = _forward_env(cfg, spec)
    inp = fz.policy_case(cfg, spec)
    control = cfg["control"] or None
    try:
        run = rollout(env, inp, cfg["activation"], K, sub, spec["tau"], clip=cfg["clip"], control=control, noise=cfg["noise"])
        assert (run["states"] is None) == (not cfg["store_states"])
        if K > 0:
            check_dynamics(run)
        else:
            _row_zero_only(run, inp, env)
        worst = 0.0
        if cfg["activation"] == "relu" or len(inp["W"]) == 1:
            check_exact(run, inp)
        else:
            worst = check_bound(run, inp)
        ratio = 0.0
        if cfg["dtype"] == "float64":
            want = hp.oracle_policy_loop(model, cfg["solver"], props, inp, spec["tau"], cfg["activation"], K=K, sub=sub, clip=cfg["clip"],
                                         control=control, noise=cfg["noise"])
            ratio = check_independent(run, inp, props, want, model, cfg["solver"], spec["tau"], f"policy draw {i}", control=control)
        assert bool(torch.isfinite(run["obs"]).all())
    except AssertionError as e:
        raise AssertionError(f"policy draw {i}: {fz.describe(cfg)}\n{e}") from e
    print(f"policy draw {i}: passed; forward error / bound {worst:.3f} (0: bit for bit), independent loop distance / allowed {ratio:.2e}")


# ---------------------------------------------------------------------------------------------------------------- (b)
def _refusal(cfg, spec):
    """The reverse entry refuses per-environment properties and the saturated PMSM by name before it touches an argument"""
    tdt = getattr(torch, cfg["dtype"])
    B = cfg["B"]
    if cfg["refusal"] == "saturated":
        env, _, _, spec = hf.saturated_env(B, tdt, cfg["solver"], "cuda")
        match = "vmap_sim_ahead_feedback_vjp: the saturated PMSM has no reverse mode"
    else:
        name = [k for k in spec["params"] if k != "deadtime"][0]
        spec["params"][name] = float(spec["params"][name]) * np.random.default_rng(cfg["seed"]).uniform(0.8, 1.2, B)
        env, _, _, _ = make_env(cfg["env_name"], B, tdt, cfg["solver"], spec=spec)
        match = r"vmap_sim_ahead_feedback_vjp: per-environment property arrays have no reverse mode \(broadcast properties only\)"
    gain = torch.zeros(env.action_dim, env._obs_dim(), dtype=tdt, device=env.device)
    with pytest.raises(ValueError, match=match):
        env.vmap_sim_ahead_feedback_vjp(None, gain, None, None, None, spec["tau"], spec["tau"] * cfg["substeps"])
    assert env.last_feedback_vjp_launch == ""
    print(f"reverse draw: refused by name ({cfg['refusal']})")


def _replicated(inp, B):
    """The same gains, one copy per environment"""
    rep = dict(inp)
    for k in ("gain", "igain"):
        if inp[k] is not None and np.ndim(inp[k]) == 2:
            rep[k] = np.broadcast_to(inp[k], (B,) + np.shape(inp[k])).copy()
    return rep


@pytest.mark.parametrize("i", SEEDS)
def test_random_closed_loop_gradient_configuration(i):
    from test_gpu_feedback_vjp import TOL, assert_batch_sum_identity, check, compare, explicit, forward

    cfg, spec = fz.draw("vjp", i)
    print("reverse draw:", fz.describe(cfg))
    if cfg["refusal"]:
        return _refusal(cfg, spec)
    env_name, solver, B, K, sub, form = cfg["env_name"], cfg["solver"], cfg["B"], cfg["K"], cfg["substeps"], cfg["gain_form"]
    tdt = getattr(torch, cfg["dtype"])
    fp32 = tdt is torch.float32
    control = cfg["control"] or None
    inp = fz.feedback_case(cfg, spec)
    if fp32:
        inp = fz.round_to(inp, np.float32)
    try:
        env, _, _, _ = make_env(env_name, B, tdt, solver, spec=spec, control_state=control)
        run = forward(env, inp, K, sub, spec["tau"], clip=cfg["clip"], control=control)
        S, A, OW = env.physical_state_dim, env.action_dim, env._obs_dim()
        group = fz.vjp_cotangents(cfg, K * sub + 1, OW, S, A, dtype=np.float32 if fp32 else None)
        got = explicit(run, group)
        seen = env.last_feedback_vjp_cotangents
        assert seen["obs"] == ("obs" in group) and seen["actions"] == ("actions" in group) and seen["z"] == ("z" in group)
        for name, key in (("states", "states"), ("last", "last_state")):
            assert seen[key] == [name in group and j in cfg[f"{name}_leaves"] for j in range(S)], (key, seen[key])
        per = None
        if form == "broadcast":
            per = assert_batch_sum_identity(run, group, got, f"reverse draw {i}")
        elif form == "mixed" and fp32:  # the broadcast gain is repeated, its gradient summed over the batch by torch
            rep = dict(run, gain=run["gain"][None].expand(B, A, OW).contiguous())
            per = explicit(rep, group)
            assert torch.equal(per["raw"][1].sum(0), got["raw"][1])
            assert np.array_equal(per["igain"], got["igain"]) and np.array_equal(per["ff"], got["ff"])
            assert all(np.array_equal(a, b) for a, b in zip(per["state0"], got["state0"]))
        drop_ff = (lambda g: dict(g, ff=None)) if cfg["feedforward"] == "none" else (lambda g: g)  # (returned all the same)
        if not fp32:
            twin, lv, out = hv.twin_run(env_name, spec, solver, inp, K, sub, clip=cfg["clip"], control=control)
            want = hv.twin_grads(lv, out, [group], OW)[0]
            dist, bound = compare(drop_ff(got), want, per_env=form == "per_env"), TOL
            check(dist, bound, f"reverse draw {i} fp64")
        else:
            # the twin on per-environment copies of the gains: its gradients per environment, and their sums
            twin, lv, out = hv.twin_run(env_name, spec, solver, _replicated(inp, B), K, sub, clip=cfg["clip"], control=control)
            want = hv.twin_grads(lv, out, [group], OW)[0]
            kd = twin.kink_distance()
            keep = np.ones(B, dtype=bool) if kd is None else kd.numpy() >= KINK_MARGIN
            excluded = 1.0 - float(np.mean(keep))
            floor = obs_floor(run["obs"].cpu().numpy().astype(np.float64), out["obs"].detach().numpy(), env_name, keep)
            bound = 32 * floor
            print(f"reverse draw {i}: excluded {excluded:.4f}, forward floor {floor:.3e}")
            assert excluded <= KINK_CAP
            dist = compare(drop_ff(got if per is None else per), want, keep)
            check(dist, bound, f"reverse draw {i} fp32 (per environment)")
            if per is not None and keep.all():  # the sums themselves
                summed = dict(want)
                for k in ("gain", "igain"):
                    if got[k] is not None and got[k].ndim == 2:
                        summed[k] = want[k].sum(0)
                check(compare(drop_ff(got), summed, per_env=False), bound, f"reverse draw {i} fp32 (summed over the batch)")
    except AssertionError as e:
        raise AssertionError(f"reverse draw {i}: {fz.describe(cfg)}\n{e}") from e
    worst = max(dist.values())
    print(f"reverse draw {i}: passed; largest distance / bound {worst / bound if bound > 0 else 0.0:.2e}")
