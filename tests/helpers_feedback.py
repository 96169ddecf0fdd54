"""Inputs and references of the closed-loop tests (tests/test_feedback_host.py, tests/test_gpu_feedback.py): seeded states, gains and
feedforward rows for every case, a float64 numpy restatement of the affine feedback policy of `vmap_sim_ahead_feedback`
(include/excenv.h excenv_feedback_t), that policy looped over `oracle.step`, and the rounding bound of the policy."""
import functools

import numpy as np

import oracle
from helpers_vjp import CASES, SOLVERS, case_spec, vjp_inputs  # noqa: F401  (CASES / SOLVERS: what the tests parametrise over)

B_MAIN, K_MAIN, SUB_MAIN = 326, 7, 3  # one full workgroup, one full wavefront and 6 lanes of a third; PMSM: substeps 1
GAIN_SCALE = 0.5                      # gains ~ N(0, GAIN_SCALE / sqrt(OW))
CLIP = (-1.0, 1.0)
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def substeps_of(env_name):
    return 1 if env_name == "pmsm" else SUB_MAIN


def obs_width(env_name, control=None):
    return oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][2] + (len(control) if control else 0)


def feedback_inputs(env_name, spec, B=B_MAIN, K=K_MAIN, seed=72, control=None, per_env_gains=True, integral=True, feedforward=True):
    """Seeded inputs of one closed-loop case, float64: dict(st, gain, igain, ff, z0, refs). States are helpers_vjp.vjp_inputs';
    gains ~ N(0, 0.5 / sqrt(OW)) ([B, A, OW], or [A, OW] for per_env_gains=False); integral gains the same, scaled by 1 / (2
    action_stepsize) so that the integrator moves by about a quarter of an observation per action row and reaches its clamp within
    the horizon; feedforward ~ U(-0.5, 0.5); the initial integrator state ~ U(-0.3, 0.3); references of the controlled fields
    inside the normalisation box."""
    A = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][1]
    OW = obs_width(env_name, control)
    st, _ = vjp_inputs(env_name, spec, B, max(K, 1), seed)
    rng = np.random.default_rng(seed + 5000)
    shape = (B, A, OW) if per_env_gains else (A, OW)
    sd = GAIN_SCALE / np.sqrt(OW)
    action_dt = spec["tau"] * substeps_of(env_name)
    out = dict(st=st, gain=rng.normal(0.0, sd, shape), igain=None, ff=None, z0=None, refs=None)
    ig = rng.normal(0.0, sd, shape) / (2.0 * action_dt)
    ff = rng.uniform(-0.5, 0.5, (B, K, A))
    z0 = rng.uniform(-0.3, 0.3, (B, A))
    if integral:
        out["igain"], out["z0"] = ig, z0
    if feedforward:
        out["ff"] = ff
    if control:
        refs = {}
        for name in control:
            lo, hi = spec["phys_norm"][name]
            refs[name] = (rng.uniform(-0.8, 0.8, B) + 1) / 2 * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) + np.asarray(lo, np.float64)
        out["refs"] = refs
    return out


def policy_np(ob, gain, igain, ff_k, z, clip, action_dt):
    """The policy on one observation row, float64 numpy, the kernel's operation order with unfused multiply-adds:
    ob [B, OW], gain / igain [A, OW] or [B, A, OW], ff_k [B, A] or None, z [B, A] or None -> (a [B, A], z' or None, the unclamped
    sums [B, A], the magnitude sum |ff| + |z| + sum |G obs| [B, A] of the action and, with igain, |z| + dt sum |Gi obs| of z')."""
    ob = np.asarray(ob, np.float64)
    B, OW = ob.shape
    g = np.broadcast_to(np.asarray(gain, np.float64), (B,) + tuple(np.shape(gain)[-2:]))
    A = g.shape[1]
    acc = np.zeros((B, A)) if ff_k is None else np.array(ff_k, np.float64)
    mag = np.abs(acc)
    if igain is not None:
        acc = acc + z
        mag = mag + np.abs(z)
    for o in range(OW):
        acc = g[:, :, o] * ob[:, o:o + 1] + acc
        mag = mag + np.abs(g[:, :, o] * ob[:, o:o + 1])
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    a = np.minimum(np.maximum(acc, lo), hi)
    z_new = zmag = None
    if igain is not None:
        h = np.broadcast_to(np.asarray(igain, np.float64), g.shape)
        zi = np.zeros((B, A))
        zimag = np.zeros((B, A))
        for o in range(OW):
            zi = h[:, :, o] * ob[:, o:o + 1] + zi
            zimag = zimag + np.abs(h[:, :, o] * ob[:, o:o + 1])
        z_new = np.minimum(np.maximum(z + action_dt * zi, lo), hi)
        zmag = np.abs(z) + action_dt * zimag
    return a, z_new, acc, mag, zmag


def oracle_closed_loop(env_name, solver, props, inp, tau, K=K_MAIN, sub=None, clip=CLIP, control=None):
    """The numpy policy looped over oracle.step in float64 ("step" semantics, solver step tau) -> dict(obs [B, N+1, OW],
    states (S x [B, N+1]), last, actions [B, K, A], z [B, A] or None, clamped: the share of action entries the clamp changed)."""
    sub = substeps_of(env_name) if sub is None else sub
    st = [np.asarray(v, np.float64) for v in inp["st"]]
    B = st[0].shape[0]
    A = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][1]
    ctl = [(n, inp["refs"][n]) for n in control] if control else None
    ob = oracle.sim_ahead(env_name, solver, st, np.zeros((B, 0, A)), props, tau, control=ctl)[0][:, 0]
    rows_o, rows_s, acts = [ob], [st], []
    z = None
    if inp["igain"] is not None:
        z = np.zeros((B, A)) if inp["z0"] is None else np.array(inp["z0"], np.float64)
    n_clamped = 0
    for k in range(K):
        a, z, raw, _, _ = policy_np(ob, inp["gain"], inp["igain"], None if inp["ff"] is None else inp["ff"][:, k], z, clip, tau * sub)
        n_clamped += int(np.sum(a != raw))
        acts.append(a)
        for _ in range(sub):
            ob, st = oracle.step(env_name, solver, st, a, props, tau, control=ctl)
            rows_o.append(ob)
            rows_s.append(st)
    S = len(st)
    return dict(obs=np.stack(rows_o, axis=1), states=[np.stack([r[j] for r in rows_s], axis=1) for j in range(S)], last=st,
                actions=np.stack(acts, axis=1) if K else np.zeros((B, 0, A)), z=z, clamped=n_clamped / max(1, B * K * A))


def policy_bounds(obs_rows, inp, clip, action_dt, dtype):
    """From the observation rows of the action rows ([B, K, OW], as the kernel returned them): the float64 actions and final
    integrator state with the allowed distance of every entry. An action entry: 2 (OW + 4) u (|ff| + |z| + sum |G obs|), nothing
    more — the error that the kernel's z carries into the action has to fit into it as well. For z the same bound runs as a
    recurrence over the rows: the clamp is 1-Lipschitz, so a row's bound is the bound carried in plus the row's own,
    2 (OW + 4) u (|z| + action_stepsize sum |Gi obs|).
    -> (actions [B, K, A], their bounds, z [B, A] or None, its bound)"""
    obs_rows = np.asarray(obs_rows, np.float64)
    B, K, OW = obs_rows.shape
    u = U[np.dtype(dtype)]
    c = 2.0 * (OW + 4) * u
    A = np.shape(inp["gain"])[-2]
    z = zb = None
    if inp["igain"] is not None:
        z = np.zeros((B, A)) if inp["z0"] is None else np.array(inp["z0"], np.float64)
        zb = np.zeros((B, A))
    acts, bounds = [], []
    for k in range(K):
        a, z_new, _, mag, zmag = policy_np(obs_rows[:, k], inp["gain"], inp["igain"], None if inp["ff"] is None else inp["ff"][:, k], z,
                                           clip, action_dt)
        acts.append(a)
        bounds.append(c * mag)
        if z is not None:
            zb = zb + c * zmag
            z = z_new
    if K == 0:
        return np.zeros((B, 0, A)), np.zeros((B, 0, A)), z, zb
    return np.stack(acts, axis=1), np.stack(bounds, axis=1), z, zb


# ---- the cases of the CPU suite's input condition and of the GPU suite --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_case(env_name, deadtime):
    """(spec, inputs) of a main case, float64, computed once per process"""
    spec = case_spec(env_name, deadtime)
    return spec, feedback_inputs(env_name, spec)


@functools.lru_cache(maxsize=None)
def oracle_case(env_name, deadtime, solver):
    """The independent fp64 closed loop of a main case, once per process (shared by the CPU input condition and GPU test 3)"""
    spec, inp = main_case(env_name, deadtime)
    B = inp["st"][0].shape[0]
    props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, B)
    return oracle_closed_loop(env_name, solver, props, inp, spec["tau"])


def saturated_env(B, dtype, solver, device, control_state=None):
    """The saturated PMSM (helpers_lut.saturating_lut) on `device` and its oracle properties in float64 -> (env, props, keep, spec)"""
    import torch

    import exciting_environments_amd as ex
    from exciting_environments_amd import EnvironmentRegistry, MotorVariant, prepare_pmsm_lut
    from helpers_lut import saturating_lut

    lut = saturating_lut()
    solv = {"euler": ex.Euler(), "rk4": ex.RK4(), "tsit5": ex.Tsit5()}[solver]
    env = EnvironmentRegistry.PMSM.make(batch_size=B, saturated=True, motor_variant=MotorVariant.BRUSA, pmsm_lut=lut, solver=solv,
                                        dtype=dtype, device=device, control_state=control_state)
    ep = env.env_properties
    params = {n: getattr(ep.static_params, n) for n in env.PARAM_FIELDS}
    pn = {n: (getattr(ep.physical_normalizations, n).min, getattr(ep.physical_normalizations, n).max) for n in env.STATE_FIELDS}
    an = {n: (getattr(ep.action_normalizations, n).min, getattr(ep.action_normalizations, n).max) for n in env.ACTION_FIELDS}
    props, keep = oracle.make_props("pmsm", params, pn, an, np.float64, B, pmsm_lut=prepare_pmsm_lut(lut))
    return env, props, keep, dict(params=params, phys_norm=pn, act_norm=an, tau=env.tau)

