"""Inputs and the float64 reference of the reverse-mode step tests (tests/test_step_vjp_host.py, tests/test_gpu_step_vjp.py).

Reference: helpers_vjp.Twin with K = 1 under "step" (one `vmap_step`), plus a float64 torch restatement of the reward of the
controlled fields below, written from the expressions of the reference's generate_reward (angles through sin / cos, other fields
through the normalised difference; PMSM's current reward -(0.5 dd^2 + 0.5 dq^2)(1 - 0.85)).

Inputs: helpers_vjp.vjp_inputs on helpers_vjp.skewed_spec, B = 257 (one full workgroup plus a one-lane tail, a multiple of no
vector width), references uniform in the normalised box."""
import numpy as np
import torch

import oracle
from helpers import ANGLE_STATES
from helpers_vjp import DT, Twin, leaves, normalize, skewed_spec, vjp_inputs

B0 = 257
SEED = 31
# the controlled fields of the twin comparisons: an angle where the model has one; PMSM: the (smooth) current reward
CONTROL = {"pendulum": ("theta", "omega"), "mass_spring_damper": ("deflection",), "cartpole": ("velocity", "theta"),
           "acrobot": ("theta_1", "omega_2"), "fluid_tank": ("height",), "pmsm": ("i_d", "i_q")}


def refs_for(env_name, control, spec, B, seed=93):
    rng = np.random.default_rng(seed)
    out = {}
    for n in control:
        lo, hi = (float(v) for v in spec["phys_norm"][n])
        out[n] = (rng.uniform(-1, 1, B) + 1) / 2 * (hi - lo) + lo
    return out


def step_inputs(env_name, deadtime, B=B0, seed=SEED, np_dtype=np.float64):
    """-> spec, state leaves S x [B], action [B, A]; np_dtype float32: fp32-representable values (returned as float32)"""
    spec = skewed_spec(env_name, deadtime)
    st, acts = vjp_inputs(env_name, spec, B, 1, seed, np_dtype=np_dtype)
    return spec, st, acts[:, 0]


def reward64(env_name, spec, control, st, refs):
    """float64 torch reward [B] of the state `st` (list of S [B] tensors) for the control sets of CONTROL"""
    fields = oracle.STATE_FIELDS[env_name]
    bounds = lambda n: tuple(float(v) for v in spec["phys_norm"][n])
    r = lambda n: torch.as_tensor(np.asarray(refs[n], dtype=np.float64))
    if env_name == "pmsm":
        assert tuple(control) == ("i_d", "i_q")
        dd = normalize(st[3], *bounds("i_d")) - normalize(r("i_d"), *bounds("i_d"))
        dq = normalize(st[4], *bounds("i_q")) - normalize(r("i_q"), *bounds("i_q"))
        return -1 * ((0.5 * dd * dd + 0.5 * dq * dq) * (1 - 0.85))
    out = torch.zeros_like(st[0])
    for n in control:
        j = fields.index(n)
        if j in ANGLE_STATES.get(env_name, []):
            out = out + -((torch.sin(st[j]) - torch.sin(r(n))) ** 2 + (torch.cos(st[j]) - torch.cos(r(n))) ** 2)
        else:
            out = out + -((normalize(st[j], *bounds(n)) - normalize(r(n), *bounds(n))) ** 2)
    return out


def twin_step(env_name, spec, solver, st_np, action_np, control=(), refs=None):
    """One twin step with a graph -> (state leaves, action [B, A] leaf, obs [B, O], new state list of [B], reward [B] or None,
    kink distance [B] or None)"""
    twin = Twin(env_name, spec, solver, "step")
    lv = leaves(st_np, True)
    act = torch.tensor(np.asarray(action_np, dtype=np.float64), dtype=DT, requires_grad=True)
    obs, _, last = twin.sim_ahead(lv, act[:, None, :], spec["tau"], 1)
    rew = reward64(env_name, spec, control, last, refs) if control else None
    return lv, act, obs[:, 1], last, rew, twin.kink_distance()


def twin_step_grads(tw, g_obs=None, g_state=None, g_rew=None):
    """Gradients of <cotangents, outputs> of a twin_step w.r.t. the action and the state leaves (numpy, zeros where unused)"""
    lv, act, obs, last, rew, _ = tw
    loss = torch.zeros((), dtype=DT)
    if g_obs is not None:
        loss = loss + (obs * torch.as_tensor(np.asarray(g_obs, dtype=np.float64)[:, :obs.shape[1]])).sum()
    if g_state is not None:
        loss = loss + sum((s * torch.as_tensor(np.asarray(g, dtype=np.float64))).sum() for s, g in zip(last, g_state) if g is not None)
    if g_rew is not None and rew is not None:
        loss = loss + (rew * torch.as_tensor(np.asarray(g_rew, dtype=np.float64).reshape(-1))).sum()
    if not loss.requires_grad:
        return np.zeros(tuple(act.shape)), [np.zeros(tuple(s.shape)) for s in lv]
    gr = torch.autograd.grad(loss, [act] + lv, allow_unused=True, retain_graph=True)
    z = lambda g, like: np.zeros(tuple(like.shape)) if g is None else g.numpy()
    return z(gr[0], act), [z(g, s) for g, s in zip(gr[1:], lv)]


def check_fp32_excluded_share():
    """The fp32 comparisons of tests/test_gpu_step_vjp.py and tests/test_gpu_linearize.py leave out the environments the twin sees
    closer than KINK_MARGIN to a kink: on their inputs (step_inputs, fp32-representable values, every model and solver) that is at
    most KINK_CAP of them."""
    from helpers_vjp import CASES, KINK_CAP, KINK_MARGIN, SOLVERS

    for env_name, deadtime in CASES:
        spec, st, act = step_inputs(env_name, deadtime, B0, np_dtype=np.float32)
        for solver in SOLVERS:
            kd = twin_step(env_name, spec, solver, [v.astype(np.float64) for v in st], act.astype(np.float64))[5]
            excluded = 0.0 if kd is None else float((kd.numpy() < KINK_MARGIN).mean())
            print(f"{env_name} dead={deadtime} {solver}: excluded {excluded:.4f}")
            assert excluded <= KINK_CAP
