"""Inputs and the independent reference of the reward reverse-mode tests (tests/test_reward_vjp_host.py, tests/test_gpu_reward_vjp.py).

Reference. The reward of row n reads the state of row n only, so its Jacobian is diagonal per leaf: the product with a reward
cotangent g is g * dR/dx elementwise, and dR/dx is a central difference of the fp64 CPU oracle (oracle.rew_trunc_term_ahead),
one read leaf perturbed at a time over the whole array, two oracle calls per leaf. Step: h = 1e-6 x (max - min) of the field,
1e-6 rad for angle fields.

Inputs (seeded, synthesised directly — no simulation): normalised states uniform in [-1.2, 1.2] denormalised with the environment's
bounds, references uniform in [-1, 1], standard-normal cotangents. PMSM with torque controlled: |tq - tr| uniform in [0, 0.009]
for 30 % of the elements and in [0.02, 1] for the rest, so that each of the torque reward's four live branches (i_s > 1; i_d > 0.2;
|d| > tol; |d| < tol) holds at least 10 % of the elements; i_n < i_s < 1 is empty by construction (i_n = 1). The expected share of
the smallest branch is (pi - 1.1735) / 5.76 x 0.3 = 0.1025: SEED is one for which every shape of the tests meets the 10 %
(branch_shares, asserted in the CPU suite).

Exclusion (PMSM torque reward only; the other rewards are smooth): an element is left out where a predicate operand, in normalised
units, lies within KINK_MARGIN = 1e-4 of its threshold (i_s vs 1, i_d vs 0.2, |d| vs 0.01) — the difference quotient straddles the
kink there — or where i_s < 1e-2 (sqrt's third derivative makes the quotient itself wrong). Expected share 4e-4 (annulus 2.2e-4,
strip 8e-5, disc 5.5e-5); at most KINK_CAP = 0.02 may be excluded."""
import functools

import numpy as np
import torch

import oracle
from helpers import ANGLE_STATES, spec_of
from helpers_vjp import KINK_CAP, KINK_MARGIN, WIDE_LANES  # noqa: F401  (the project's figures)

ROWS = 8
NARROW_B = 1001
SEED = 5
MIN_BRANCH_SHARE = 0.10
ORIGIN_MARGIN = 1e-2


def wide_b(elem):
    """B = V x WIDE_LANES: a full workgroup, a full wavefront and a ragged third of 16-byte lanes"""
    return (16 // elem) * WIDE_LANES


def control_sets(env_name):
    """Every single field, one multi-field set, no control; PMSM also the sets that switch its two reward terms"""
    fields = oracle.STATE_FIELDS[env_name]
    sets = [(f,) for f in fields]
    if env_name == "pmsm":
        sets += [("i_d", "i_q"), ("i_d", "i_q", "torque"), ("omega_el", "torque", "epsilon")]
    elif len(fields) > 1:
        sets += [tuple(fields[::2]) if len(fields) > 2 else tuple(fields)]
    return sets + [()]


def expected_reads(env_name, control):
    fields = oracle.STATE_FIELDS[env_name]
    if env_name != "pmsm":
        return [f in control for f in fields]
    cur = "i_d" in control and "i_q" in control
    tq = "torque" in control
    return [(f in ("i_d", "i_q") and (cur or tq)) or (f == "torque" and tq) for f in fields]


def normalize(x, lo, hi):
    return 2 * (x - lo) / (hi - lo) - 1


def denormalize(x, lo, hi):
    return (x + 1) / 2 * (hi - lo) + lo


@functools.lru_cache(maxsize=None)
def reward_inputs(env_name, control, B, rows=ROWS, elem=8, seed=SEED):
    """-> dict(leaves: S x [B, rows] fp64, refs: {name: [B] fp64}, g: [B, rows - 1] fp64). elem = 4: every value is
    fp32-representable (the same numbers go to an fp32 kernel and, widened, to the fp64 oracle). Cached: treat as read-only."""
    spec = spec_of(env_name)
    fields = oracle.STATE_FIELDS[env_name]
    rng = np.random.default_rng(seed)
    cast = (lambda a: a.astype(np.float32).astype(np.float64)) if elem == 4 else (lambda a: a)
    norm = {f: rng.uniform(-1.2, 1.2, (B, rows)) for f in fields}
    refn = {f: rng.uniform(-1.0, 1.0, B) for f in fields}
    g = rng.normal(size=(B, max(rows - 1, 0)))
    small = rng.uniform(0.0, 1.0, (B, rows)) < 0.3
    delta = np.where(small, rng.uniform(0.0, 0.009, (B, rows)), rng.uniform(0.02, 1.0, (B, rows)))
    sign = np.where(rng.uniform(0.0, 1.0, (B, rows)) < 0.5, -1.0, 1.0)
    if env_name == "pmsm" and "torque" in control:
        norm["torque"] = refn["torque"][:, None] + sign * delta
    bounds = {f: tuple(float(v) for v in spec["phys_norm"][f]) for f in fields}
    refs = {f: cast(denormalize(refn[f], *bounds[f])) for f in control}
    leaves = [cast(denormalize(norm[f], *bounds[f])) for f in fields]
    for a in leaves + list(refs.values()) + [g]:
        a.setflags(write=False)
    return dict(leaves=leaves, refs=refs, g=cast(g) if g.size else g)


def _props_arrays(env_name, spec, n, per_env=None):
    """oracle properties for n flattened elements; per_env: {(field, 'max'|'min'): [n] array} overrides"""
    phys = {}
    for f, (lo, hi) in spec["phys_norm"].items():
        lo = per_env.get((f, "min"), lo) if per_env else lo
        hi = per_env.get((f, "max"), hi) if per_env else hi
        phys[f] = (lo, hi)
    return oracle.make_props(env_name, spec["params"], phys, spec["act_norm"], np.float64, n)


def oracle_reward(env_name, control, leaves, refs, per_env=None):
    """fp64 oracle reward of every element of [B, rows] leaves (row 0 included: each element is an oracle environment whose
    row 1 holds it). refs[name]: [B] or [B, rows]; per_env: {(field, 'min'|'max'): [B]} property arrays."""
    B, rows = leaves[0].shape
    n = B * rows
    spec = spec_of(env_name)
    flat = lambda a: np.ascontiguousarray(np.broadcast_to(a if np.ndim(a) == 2 else np.asarray(a)[:, None], (B, rows))).reshape(n)
    pe = None if per_env is None else {k: flat(v) for k, v in per_env.items()}
    props, keep = _props_arrays(env_name, spec, n, pe)
    st = [np.repeat(flat(l)[:, None], 2, axis=1) for l in leaves]
    ctl = [(name, flat(refs[name])) for name in control]
    r, _, _ = oracle.rew_trunc_term_ahead(env_name, st, props, control=ctl or None)
    return r.reshape(B, rows)


def field_step(env_name, j, spec=None, per_env=None):
    spec = spec or spec_of(env_name)
    f = oracle.STATE_FIELDS[env_name][j]
    if j in ANGLE_STATES.get(env_name, []) and env_name != "pmsm":
        return 1e-6
    lo, hi = spec["phys_norm"][f]
    if per_env:
        lo, hi = per_env.get((f, "min"), lo), per_env.get((f, "max"), hi)
    return 1e-6 * (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))


def oracle_grads(env_name, control, leaves, refs, g, per_env=None):
    """-> per state leaf the [B, rows] product g * dR/dx by central differences of the oracle (row 0: zero), None where the reward
    does not read the leaf"""
    reads = expected_reads(env_name, control)
    B, rows = leaves[0].shape
    out = []
    for j, read in enumerate(reads):
        if not read:
            out.append(None)
            continue
        h = field_step(env_name, j, per_env=per_env)
        h = h[:, None] if np.ndim(h) == 1 else h
        up = [l if q != j else l + h for q, l in enumerate(leaves)]
        dn = [l if q != j else l - h for q, l in enumerate(leaves)]
        d = (oracle_reward(env_name, control, up, refs, per_env) - oracle_reward(env_name, control, dn, refs, per_env)) / (2 * h)
        gr = np.zeros((B, rows))
        gr[:, 1:] = g * d[:, 1:]
        out.append(gr)
    return out


def _torque_operands(env_name, leaves, refs):
    spec = spec_of(env_name)
    n = lambda f, x: normalize(x, *[float(v) for v in spec["phys_norm"][f]])
    fields = oracle.STATE_FIELDS[env_name]
    i_d, i_q = n("i_d", leaves[fields.index("i_d")]), n("i_q", leaves[fields.index("i_q")])
    tq = n("torque", leaves[fields.index("torque")])
    tr = n("torque", np.asarray(refs["torque"]))
    tr = tr[:, None] if tr.ndim == 1 else tr
    return i_d, i_q, np.sqrt(i_d * i_d + i_q * i_q), np.abs(tq - tr)


def keep_mask(env_name, control, leaves, refs):
    """[B, rows] bool: the elements the comparison keeps (everything but the PMSM torque reward's kinks)"""
    B, rows = leaves[0].shape
    if not (env_name == "pmsm" and "torque" in control):
        return np.ones((B, rows), dtype=bool)
    i_d, _, i_s, ad = _torque_operands(env_name, leaves, refs)
    near = (np.abs(i_s - 1.0) < KINK_MARGIN) | (np.abs(i_d - 0.2) < KINK_MARGIN) | (np.abs(ad - 0.01) < KINK_MARGIN) | (i_s < ORIGIN_MARGIN)
    return ~near


def branch_shares(env_name, leaves, refs):
    """Shares of the rewarded elements (rows 1..) in the torque reward's four live branches, and in the empty one"""
    i_d, _, i_s, ad = _torque_operands(env_name, leaves, refs)
    i_d, i_s, ad = i_d[:, 1:], i_s[:, 1:], ad[:, 1:]
    inside = i_s < 1.0
    return dict(over=float((i_s > 1.0).mean()), i_d_plus=float((inside & (i_d > 0.2)).mean()),
                far=float((inside & (i_d < 0.2) & (ad > 0.01)).mean()), near=float((inside & (i_d < 0.2) & (ad < 0.01)).mean()),
                empty=float(((i_s < 1.0) & (i_s > 1.0)).mean()))


def check_coverage_and_cap(env_name, control, leaves, refs):
    """The assertions every comparison on the PMSM torque reward makes about its own inputs; returns the keep mask"""
    keep = keep_mask(env_name, control, leaves, refs)
    excluded = 1.0 - float(keep.mean())
    assert excluded <= KINK_CAP, f"{excluded:.4f} of the elements excluded"
    if env_name == "pmsm" and "torque" in control:
        sh = branch_shares(env_name, leaves, refs)
        assert sh["empty"] == 0.0
        for k in ("over", "i_d_plus", "far", "near"):
            assert sh[k] >= MIN_BRANCH_SHARE, (k, sh)
    return keep


def rel_dist(got, want, keep):
    """max |got - want| over the kept elements, relative to the leaf's largest magnitude"""
    scale = float(np.max(np.abs(want[keep])))
    return float(np.max(np.abs(got[keep] - want[keep]))) / scale if scale > 0 else float(np.max(np.abs(got[keep])))


def tensor(a, env=None):
    """A fresh tensor over a copy of `a` (the cached inputs are read-only), in the environment's dtype on its device"""
    t = torch.from_numpy(np.array(a, dtype=np.float64, order="C"))
    return t if env is None else t.to(device=env.device, dtype=env.dtype)


def make_states(env, data, layout="lane", refs_along_rows=False):
    """The package's State pytree over the inputs: physical leaves [B, rows] lane-major (layout='lane': strides (1, B)) or
    row-major (layout='row'), reference leaves [B, rows] — broadcast views of [B] values, or row-major [B, rows] copies
    (refs_along_rows: `data['refs']` then holds [B, rows] arrays)."""
    B, rows = data["leaves"][0].shape
    t = lambda a: tensor(a, env)
    if layout == "lane":
        leaves = [t(l.T).t() for l in data["leaves"]]
    else:
        leaves = [t(l) for l in data["leaves"]]
    ref = {}
    for n in env.STATE_FIELDS:
        if n in data["refs"]:
            r = np.asarray(data["refs"][n])
            ref[n] = t(r) if r.ndim == 2 else t(r)[:, None].expand(B, rows)
        else:
            ref[n] = torch.full((B, 1), float("nan"), dtype=env.dtype, device=env.device).expand(B, rows)
    return env.State(physical_state=env.PhysicalState(*leaves), PRNGKey=None, additions=None, reference=env.PhysicalState(**ref))


def to_np(ps, fields):
    return [None if getattr(ps, n) is None else getattr(ps, n).detach().cpu().numpy().astype(np.float64) for n in fields]
