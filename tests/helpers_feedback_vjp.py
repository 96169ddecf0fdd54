"""The float64 torch closed loop ("twin") of the reverse-mode closed-loop tests (tests/test_feedback_vjp_host.py,
tests/test_gpu_feedback_vjp.py): helpers_vjp.Twin's own methods (constraint, rk_step, post, observe: the "step" branch of its
sim_ahead, one step at a time) with the affine feedback policy of `vmap_sim_ahead_feedback` written in DESIGN.md §4.11's operation
order and helpers_vjp.clamp0 (derivative 0 on and outside the bounds). Gradients come from torch.autograd.grad on the CPU.

The twin records, per environment, the smallest relative distance of every unclamped action sum acc_k and of every unclamped
integrator sum z_k + adt zi_k to a clamp bound; that distance joins the twin's own kink distance (Twin.kinks), so one mask covers
the model's kinks and the policy's.

Inputs are helpers_feedback.feedback_inputs'; the main case is B_MAIN = 326, K_MAIN = 7, substeps 3 (PMSM: 1)."""
import functools

import numpy as np
import torch

import helpers_feedback as hf
from helpers_vjp import DT, KINK_CAP, KINK_MARGIN, Twin, clamp0, denormalize, normalize  # noqa: F401  (the caps: for the tests)

LEAF_NAMES = ("state0", "gain", "igain", "ff", "z0")


def twin_step(twin, st, a, dt):
    """One solver step of the "step" semantics from the state `st` (list of S [B] leaves) under the normalised action `a` (list of
    A [B] tensors): the statements of Twin.sim_ahead's "step" branch."""
    st = list(st)
    if twin.env == "pmsm":
        deadtime = twin.P["deadtime"]
        uc = twin.constraint(a, st[2], st[6], deadtime)
        if deadtime > 0:
            u = [st[0], st[1]]
            st[0], st[1] = uc
        else:
            u = uc
        y = twin.rk_step([st[3], st[4], st[2]], u, u, dt, st[6])
        st[3], st[4], st[2] = y
    else:
        u = [denormalize(a[0], twin.amin[0], twin.amax[0])]
        st = twin.rk_step(st, u, u, dt)
    return twin.post(st)


def closed_loop(twin, st, gain, igain, ff, z0, K, sub, clip, tau, refs=None, control=None):
    """st: list of S [B] tensors; gain / igain: [A, OW] or [B, A, OW] tensors (igain may be None); ff: [B, K, A] or None; z0: [B, A]
    or None (zeros); refs: {field: [B] array} of the controlled fields `control` -> dict(obs [B, N+1, OW], states (S x [B, N+1]),
    last (S x [B]), actions [B, K, A], z [B, A] or None, clamped: share of action entries the clamp changed, z_clamped: number of
    integrator entries its clamp changed)"""
    twin.kinks, twin.clips, twin.levels = [], [], []
    B = st[0].shape[0]
    lo, hi = (-np.inf, np.inf) if clip is None else (float(clip[0]), float(clip[1]))
    cref = []
    for name in (control or []):
        j = twin.fields.index(name)
        cref.append(normalize(torch.as_tensor(np.asarray(refs[name], np.float64), dtype=DT), twin.smin[j], twin.smax[j]))
    g = gain.expand((B,) + tuple(gain.shape[-2:]))
    h = None if igain is None else igain.expand((B,) + tuple(igain.shape[-2:]))
    A, OW = g.shape[1], g.shape[2]
    z = None
    if h is not None:
        z = torch.zeros((B, A), dtype=DT) if z0 is None else z0
    adt = float(tau) * sub
    rows, acts = [], []
    n_clamped = n_zclamped = 0

    def bound_distance(x):  # [B, A] -> [B]: the smallest relative distance of a component to a clamp bound
        if clip is None:
            return
        d = torch.minimum((x.detach() - lo).abs(), (x.detach() - hi).abs()) / (hi - lo)
        twin.kinks.append(d.min(dim=1).values)

    def observe(s):
        ob = twin.observe(s)
        return torch.cat([ob] + [c[:, None] for c in cref], dim=1) if cref else ob

    st = list(st)
    obs_rows = []
    for k in range(K):
        ob = observe(st)
        acc = torch.zeros((B, A), dtype=DT) if ff is None else ff[:, k]
        if h is not None:
            acc = acc + z
        for o in range(OW):
            acc = g[:, :, o] * ob[:, o:o + 1] + acc
        bound_distance(acc)
        a = clamp0(acc, lo, hi)
        n_clamped += int(((acc.detach() <= lo) | (acc.detach() >= hi)).sum())
        if h is not None:
            zi = torch.zeros((B, A), dtype=DT)
            for o in range(OW):
                zi = h[:, :, o] * ob[:, o:o + 1] + zi
            zs = z + adt * zi
            bound_distance(zs)
            n_zclamped += int(((zs.detach() <= lo) | (zs.detach() >= hi)).sum())
            z = clamp0(zs, lo, hi)
        acts.append(a)
        for s in range(sub):
            rows.append(list(st))
            obs_rows.append(ob if s == 0 else observe(st))
            st = twin_step(twin, st, [a[:, q] for q in range(A)], float(tau))
    rows.append(list(st))
    obs_rows.append(observe(st))
    S = len(st)
    return dict(obs=torch.stack(obs_rows, dim=1), states=[torch.stack([r[j] for r in rows], dim=1) for j in range(S)], last=st,
                actions=torch.stack(acts, dim=1) if K else torch.zeros((B, 0, A), dtype=DT), z=z,
                clamped=n_clamped / max(1, B * K * A), z_clamped=n_zclamped)


def leaves_of(inp, requires_grad=True):
    """The differentiable inputs of a case as float64 torch leaves -> dict(st=[...], gain, igain, ff, z0) (None where absent)"""
    t = lambda v: None if v is None else torch.tensor(np.asarray(v, np.float64), dtype=DT, requires_grad=requires_grad)
    return dict(st=[t(v) for v in inp["st"]], gain=t(inp["gain"]), igain=t(inp["igain"]), ff=t(inp["ff"]), z0=t(inp["z0"]))


def twin_run(env_name, spec, solver, inp, K, sub, clip=hf.CLIP, control=None):
    """-> (twin, leaves, outputs of closed_loop) with the graph alive"""
    twin = Twin(env_name, spec, solver, "step")
    lv = leaves_of(inp)
    out = closed_loop(twin, lv["st"], lv["gain"], lv["igain"], lv["ff"], lv["z0"], K, sub, clip, spec["tau"], refs=inp["refs"],
                      control=control)
    return twin, lv, out


def loss_of(out, group, O):
    """<cotangents, outputs> for one cotangent group: dict with any of obs [B, N+1, OW], states (S x [B, N+1] or None), last (S x [B]
    or None), actions [B, K, A], z [B, A]. The control columns of the obs cotangent multiply constants."""
    loss = torch.zeros((), dtype=DT)
    t = lambda v: torch.as_tensor(np.asarray(v, np.float64), dtype=DT)
    if group.get("obs") is not None:
        loss = loss + (out["obs"] * t(group["obs"])).sum()
    if group.get("states") is not None:
        loss = loss + sum((s * t(g)).sum() for s, g in zip(out["states"], group["states"]) if g is not None)
    if group.get("last") is not None:
        loss = loss + sum((s * t(g)).sum() for s, g in zip(out["last"], group["last"]) if g is not None)
    if group.get("actions") is not None and out["actions"].shape[1] > 0:
        loss = loss + (out["actions"] * t(group["actions"])).sum()
    if group.get("z") is not None and out["z"] is not None:
        loss = loss + (out["z"] * t(group["z"])).sum()
    return loss


def twin_grads(lv, out, groups, O):
    """Gradients for several cotangent groups over one forward graph -> list of dict(state0=[S x [B]], gain, igain, ff, z0) in
    float64 numpy; None where the input is absent, zeros where the loss does not reach a present one."""
    wrt = list(lv["st"]) + [lv[n] for n in ("gain", "igain", "ff", "z0") if lv[n] is not None]
    res = []
    for group in groups:
        loss = loss_of(out, group, O)
        if loss.grad_fn is None:
            gr = [None] * len(wrt)
        else:
            gr = torch.autograd.grad(loss, wrt, allow_unused=True, retain_graph=True)
        z = [np.zeros(tuple(w.shape)) if g is None else g.numpy() for g, w in zip(gr, wrt)]
        S = len(lv["st"])
        d = dict(state0=z[:S])
        rest = iter(z[S:])
        for n in ("gain", "igain", "ff", "z0"):
            d[n] = next(rest) if lv[n] is not None else None
        res.append(d)
    return res


def cotangent_groups(rng, B, rows, OW, S, K, A, integral=True):
    """The four groups of the GPU test: all; grad_last_state alone; grad_obs alone; grad_actions + grad_z alone"""
    g_obs = rng.normal(size=(B, rows, OW))
    g_states = [rng.normal(size=(B, rows)) for _ in range(S)]
    g_last = [rng.normal(size=B) for _ in range(S)]
    g_act = rng.normal(size=(B, K, A))
    g_z = rng.normal(size=(B, A)) if integral else None
    return [dict(obs=g_obs, states=g_states, last=g_last, actions=g_act, z=g_z), dict(last=g_last), dict(obs=g_obs),
            dict(actions=g_act, z=g_z)]


@functools.lru_cache(maxsize=None)
def main_twin(env_name, deadtime, solver):
    """The twin's closed loop of a main case (helpers_feedback.main_case), once per process -> (spec, inp, twin, leaves, out)"""
    spec, inp = hf.main_case(env_name, deadtime)
    twin, lv, out = twin_run(env_name, spec, solver, inp, hf.K_MAIN, hf.substeps_of(env_name))
    return spec, inp, twin, lv, out
