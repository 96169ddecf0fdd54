"""One description of "off the fast path" for the cold-path tests (tests/test_cold_paths_host.py, tests/test_gpu_cold_forward.py,
tests/test_gpu_cold_reverse.py and the mixed-wave probes of tests/test_gpu_parity.py). Nothing here needs a GPU.

csrc/devmath.hpp guards its slow paths with a wave-uniform ballot; helpers.random_state draws angles inside +-0.9 pi and every other
leaf inside its normalisation box, so no kernel-level test ever took one with mixed lanes. Here the special values are defined per
KIND, placed in a lane pattern in which wave-uniform and mixed waves both occur (special_envs), and written into otherwise random
inputs (build): `special` holds them, `plain` is the same arrays with an ordinary random value in every special environment.

No value below is chosen to make a kernel fault, and none reaches an address unclamped: the only data-dependent addresses of the
library are the saturated PMSM's table cells (models.hpp PmsmSat::find clamps the guessed cell to [0, n - 2], maps NaN to cell 0 and
bounds both walks by the cell index), and that model gets finite currents far outside its tables and NaN only (SATURATED_KINDS)."""
import math

import numpy as np

import oracle
from helpers import ANGLE_STATES, random_state

TWO_PI = 2 * math.pi
# ---- the thresholds, restated from csrc/devmath.hpp ----------------------------------------------------------------------------
TRIG32_LIMIT = 65536.0                 # sincos_t(float): `big = !(xabs(x) <= 65536.0f)` -> sincos_lib
MOD_QUOTIENT = 4194304.0               # pymod_two_pi: `big = !(q < T(4194304.0))`, q = trunc(|x| * inv_two_pi) -> xfmod_slow
MOD_LIMIT = MOD_QUOTIENT * TWO_PI      # ... i.e. |x| >= 2.64e7 (wrap_angle passes x = theta + pi)
QUAD64_LIMIT = 2.0 ** 31 * math.pi / 2  # sincos_lean: where the former `(int)n` left the int range, |x| >= 3.37e9
DIV_WINDOW = {np.float32: 60, np.float64: 400}  # InvDivLimits: quotient exponents in [-60, 60) / [-400, 400), zero outside
HUGE = {np.float32: 1e30, np.float64: 1e200}

ANGLE_KINDS = ("turns", "trig32", "mod", "quad64")
LEAF_KINDS = ("zero", "huge", "nan", "inf")
KINDS = {
    "turns": "wrapped angle + 2 pi k, |theta| ~ 6e3: nothing cold, an unwrapped angle",
    "trig32": "|theta| in (65536, 1e5): sincos_lib in fp32",
    "mod": "|theta| in (3e7, 1e8): xfmod_slow",
    "quad64": "|theta| ~ 1e10, fp64 only: past the int range of sincos_lean's former quadrant",
    "zero": "a non-angle leaf exactly 0 / exactly at its lower bound: a zero quotient in InvDiv",
    "huge": "1e30 (fp32) / 1e200 (fp64) on a non-angle leaf: quotient window exceeded",
    "nan": "NaN on a non-angle leaf", "inf": "+-inf on a non-angle leaf",
    "far": "saturated PMSM only: a finite current far outside the tables (the clamped cell search)",
}
NONFINITE_KINDS = ("huge", "nan", "inf")  # environments whose outputs may be inf / NaN
SATURATED_KINDS = ("turns", "trig32", "mod", "quad64", "far", "nan")
REVERSE_KINDS = ("turns", "trig32", "mod", "quad64", "zero")
FAR_CURRENT = 5.0e4  # A; helpers_lut tables end at 250 A (2000 A for the global-memory ones)


def kinds_for(env_name, dtype, saturated=False, reverse=False):
    """The kinds that apply to a model in a number format, in the table's order"""
    base = SATURATED_KINDS if saturated else (REVERSE_KINDS if reverse else ANGLE_KINDS + LEAF_KINDS)
    out = [k for k in base if not (k in ANGLE_KINDS and env_name not in ANGLE_STATES)]
    return [k for k in out if not (k == "quad64" and np.dtype(dtype) == np.float32)]


# ---- the lane pattern ------------------------------------------------------------------------------------------------------------
def special_envs(B, V):
    """[(slot name, [environments])] with lane = env // V and wave = lane // 64: environment 0; the first environment of lane 31;
    the last of lane 63 (wave 0 is mixed); one in the middle of wave 1; none in wave 2; every environment of wave 3 (uniform);
    environment B - 1, the ragged tail. Needs at least four waves and a tail beyond them."""
    lanes = -(-B // V)
    assert lanes > 256 and B - 1 >= 256 * V, (B, V)
    return [("env0", [0]), ("lane31", [31 * V]), ("lane63", [63 * V + V - 1]), ("wave1", [(64 + 32) * V + V // 2]),
            ("wave3", list(range(192 * V, 256 * V))), ("tail", [B - 1])]


def assignment(B, V, kinds, uniform):
    """{environment: (kind, running number)}: the single slots take the kinds in turn (starting after `uniform`, so that the mixed
    waves hold other kinds than the uniform one wherever there are several), wave 3 holds `uniform` in every environment"""
    assert uniform in kinds
    out, n = {}, 0
    start = list(kinds).index(uniform) + 1
    for slot, envs in special_envs(B, V):
        for e in envs:
            kind = uniform if slot == "wave3" else kinds[(start + n) % len(kinds)]
            out[e] = (kind, n)
            n += 1
    return out


def angle_value(kind, n, rng):
    sign = -1.0 if n % 2 else 1.0
    if kind == "turns":
        return rng.uniform(-0.9, 0.9) * math.pi + sign * TWO_PI * 955
    lo, hi = {"trig32": (6.6e4, 9.9e4), "mod": (3.1e7, 9.9e7), "quad64": (0.9e10, 1.1e10)}[kind]
    return sign * rng.uniform(lo, hi)


def leaf_value(kind, n, lo, dtype):
    sign = -1.0 if n % 2 else 1.0
    if kind == "zero":
        return float(lo) if n % 2 else 0.0
    return {"huge": sign * HUGE[np.dtype(dtype).type], "nan": math.nan, "inf": sign * math.inf, "far": sign * FAR_CURRENT}[kind]


def leaf_targets(env_name, saturated=False, reverse=False):
    """The non-angle leaves a leaf kind is written to, taken in turn. PMSM: the currents and the speed (the torque leaf is
    recomputed from the currents and never read; the saturated model: the currents only, see the module text). Reverse: the last
    leaf (an angular velocity; cart-pole's velocity leaf would sit on the kink of sign() at 0)."""
    S = len(oracle.STATE_FIELDS[env_name])
    if saturated:
        return [3, 4]
    if reverse:
        return [S - 1]
    if env_name == "pmsm":
        return [3, 4, 6, 0]
    return [j for j in range(S) if j not in ANGLE_STATES.get(env_name, [])]


def build(env_name, spec, dtype, B, V, uniform, seed, saturated=False, reverse=False, plain=None, kinds=None):
    """-> dict(special, plain: S x [B] in the number format; mask [B]: the special environments; kind [B]: their kind ('' else);
    written [S, B]: the leaves that hold a special value). plain: the arrays to start from (default helpers.random_state)."""
    npdt = np.dtype(dtype).type
    kinds = kinds or kinds_for(env_name, dtype, saturated, reverse)
    plain = [np.array(v, dtype=npdt) for v in (plain if plain is not None else random_state(env_name, B, npdt, spec, seed))]
    special = [v.copy() for v in plain]
    rng = np.random.default_rng(seed + 77)
    mask, kind_of = np.zeros(B, dtype=bool), np.array([""] * B, dtype=object)
    written = np.zeros((len(plain), B), dtype=bool)
    targets = leaf_targets(env_name, saturated, reverse)
    fields = oracle.STATE_FIELDS[env_name]
    for e, (kind, n) in sorted(assignment(B, V, kinds, uniform).items()):
        mask[e], kind_of[e] = True, kind
        if kind in ANGLE_KINDS:
            for j in ANGLE_STATES[env_name]:
                special[j][e] = npdt(angle_value(kind, n + j, rng))
                written[j, e] = True
        else:
            j = targets[n % len(targets)]
            lo = np.broadcast_to(np.asarray(spec["phys_norm"][fields[j]][0], dtype=np.float64), (B,))[e]
            special[j][e] = npdt(leaf_value(kind, n, lo, npdt))
            written[j, e] = True
    return dict(special=special, plain=plain, mask=mask, kind=kind_of, written=written, V=V, uniform=uniform)


def special_references(refs, names, env_name, mask, dtype, seed):
    """References of the controlled fields for the gym forms: an angle field's reference takes a `turns` value in the even special
    environments and a `trig32` value in the odd ones (the reward reads sin and cos of state and reference)"""
    npdt = np.dtype(dtype).type
    rng = np.random.default_rng(seed + 78)
    out = [np.array(r, dtype=npdt) for r in refs]
    fields = oracle.STATE_FIELDS[env_name]
    for q, name in enumerate(names):
        if fields.index(name) in ANGLE_STATES.get(env_name, []):
            for n, e in enumerate(np.flatnonzero(mask)):
                out[q][e] = npdt(angle_value("trig32" if n % 2 else "turns", n, rng))
    return out


def one_ulp(leaves, written, direction):
    """The special leaves moved by one ulp of their own number format (direction +1 / -1), everything else as it is"""
    out = []
    for v, w in zip(leaves, written):
        v = v.copy()
        v[w] = np.nextafter(v[w], np.asarray(direction * np.inf, dtype=v.dtype))
        out.append(v)
    return out


# ---- what the host test asserts about the values (after rounding to the number format) ---------------------------------------------
def crosses(kind, value, lo, hi, dtype):
    """True where `value` of a leaf with the normalisation range [lo, hi] lies beyond the threshold its kind is meant to cross"""
    npdt = np.dtype(dtype).type
    v = float(value)
    if kind == "turns":
        return math.pi < abs(v) <= TRIG32_LIMIT
    if kind == "trig32":
        return TRIG32_LIMIT < abs(v) < MOD_LIMIT - math.pi
    if kind == "mod":
        return math.trunc(float(npdt(abs(npdt(v + npdt(math.pi))) * npdt(1 / TWO_PI)))) >= MOD_QUOTIENT and abs(v) < QUAD64_LIMIT
    if kind == "quad64":
        return abs(v) >= QUAD64_LIMIT and npdt is np.float64
    q = npdt(2) * (npdt(v) - npdt(lo)) / (npdt(hi) - npdt(lo))  # the quotient of normalize()
    if kind == "zero":
        return v == 0.0 or q == 0.0
    if kind in ("huge", "far"):
        return np.isfinite(v) and (abs(float(q)) >= 2.0 ** DIV_WINDOW[npdt] if kind == "huge" else abs(v) > 10 * max(abs(lo), abs(hi)))
    return not np.isfinite(v)


def inside(values, lo, hi, dtype, angle):
    """[B] bool: where an ordinary value takes every fast path — a wrapped angle, a normalisation quotient inside the window.
    values [B]; lo, hi: the leaf's normalisation range, scalars or [B]"""
    npdt = np.dtype(dtype).type
    v = np.asarray(values, dtype=npdt)
    if angle:  # below the lowest angle threshold (and so below MOD_LIMIT and QUAD64_LIMIT); the per-environment boxes of the general
        return np.abs(v.astype(np.float64)) <= 4.0  # kernel's case reach 1.2 pi, so "wrapped" would ask too much: within 4 rad
    lo, hi = np.asarray(lo, dtype=np.float64).astype(npdt), np.asarray(hi, dtype=np.float64).astype(npdt)
    q = np.abs((npdt(2) * (v - lo) / (hi - lo)).astype(np.float64))  # the quotient of normalize()
    return np.isfinite(v) & (2.0 ** -DIV_WINDOW[npdt] <= q) & (q < 2.0 ** DIV_WINDOW[npdt])


def all_inside(env_name, spec, leaves, dtype):
    """-> the (field, environment, value) of the first plain value outside a threshold, or None"""
    for j, f in enumerate(oracle.STATE_FIELDS[env_name]):
        lo, hi = spec["phys_norm"][f]
        ok = inside(leaves[j], lo, hi, dtype, j in ANGLE_STATES.get(env_name, []))
        if not ok.all():
            e = int(np.flatnonzero(~ok)[0])
            return f, e, leaves[j][e]
    return None


def wave_summary(mask, V, period=1):
    """Per wave (lane = env // V, 64 lanes): 'clean', 'mixed' or 'uniform' (every active lane holds at least one special environment).
    period > 1: the map of sim_ahead_emr_kernel instead (kernels_emr.hpp: `env = env0 + P * lane`, `env0 = (wave / P) * 64 * P +
    wave % P`, one environment per lane) — its waves interleave, so the pattern of special_envs does not hold there."""
    B = mask.shape[0]
    env = np.arange(B)
    if period > 1:
        assert V == 1
        group, within = env // (64 * period), env % (64 * period)
        wave, lane = group * period + within % period, within // period
    else:
        wave, lane = env // V // 64, env // V % 64
    slot = wave * 64 + lane
    waves = int(wave.max()) + 1
    active = np.bincount(np.unique(slot) // 64, minlength=waves)
    special = np.bincount(np.unique(slot[mask]) // 64, minlength=waves)
    return ["uniform" if s == a > 0 else ("mixed" if s else "clean") for s, a in zip(special, active)]


# ---- comparing outputs that may hold NaN / inf ---------------------------------------------------------------------------------------
def nonfinite_equal(got, want):
    """NaN at the same positions, inf at the same positions with the same sign"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.where(np.isinf(got), got, 0), np.where(np.isinf(want), want, 0)))


def finite_distance(got, want, cols=(), period=2.0):
    """Largest |got - want| / (1 + |want|) over the entries finite on both sides, the columns `cols` (last axis) on the circle"""
    got, want = np.array(got, dtype=np.float64), np.array(want, dtype=np.float64)
    ok = np.isfinite(got) & np.isfinite(want)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
        for c in cols:
            d[..., c] = np.minimum(d[..., c], np.abs(period - d[..., c]))
        d = d / (1.0 + np.abs(want))
    return float(d[ok].max()) if ok.any() else 0.0


# ====================================================================== the reverse cases (tests/test_gpu_cold_reverse.py)
# Shared with tests/test_cold_paths_host.py, which runs the twin on them, asserts the kink cap and prints the twin's own spread.
# (The closed loop's reverse mode: feedback_twin_reference at the end of this file.)
REV_MODELS = [("pendulum", None), ("cartpole", None), ("acrobot", None), ("pmsm", 0), ("pmsm", 1)]
REV_SOLVERS = ["euler", "rk4", "tsit5"]
REV_DTYPES = ["float32", "float64"]
REV_K = 3
REV_LANES = 326  # helpers_vjp.WIDE_LANES: B = V * 326, so that wave 3 exists at every lane width (326 environments at V = 2 are 163 lanes)
REV_SEED = 172


def reverse_cases():
    return [(e, d, s, t) for e, d in REV_MODELS for s in REV_SOLVERS for t in REV_DTYPES]


def reverse_id(case):
    e, d, s, t = case
    return f"{e}{'' if d is None else f'_deadtime{d}'}-{s}-{t}"


def reverse_forms(env_name, dtype, solver):
    """(semantics, environments per lane, substeps) of one case: V = 1 and the wide form where helpers_vjp.WIDE_CASES has one"""
    from helpers_vjp import vjp_wide_ok

    elem = np.dtype(dtype).itemsize
    widths = [1] + ([16 // elem] if vjp_wide_ok(env_name, elem, solver) else [])
    subs = (1,) if env_name == "pmsm" else (1, 2)
    return [(sem, V, sub) for sem in ("ahead", "step") for V in widths for sub in subs]


def uniform_kind(case, kinds, shift=0):
    """The kind wave 3 holds in a case: they take turns over the case list, so that each is the uniform one somewhere"""
    return kinds[(reverse_cases().index(case) + shift) % len(kinds)]


_REV = {}


def reverse_setup(env_name, deadtime, dtype, V, K=REV_K, uniform=None, kinds=None, seed=REV_SEED):
    """-> spec, build() of the initial states (helpers_vjp.vjp_inputs on skewed_spec with the specials written in), actions [B, K, A]"""
    from helpers_vjp import skewed_spec, vjp_inputs

    key = (env_name, deadtime, np.dtype(dtype).name, V, K, uniform, tuple(kinds or ()), seed)
    if key not in _REV:
        spec = skewed_spec(env_name, deadtime)
        npdt = np.dtype(dtype).type
        B = V * REV_LANES
        st, acts = vjp_inputs(env_name, spec, B, K, seed, np_dtype=npdt)
        all_kinds = kinds or kinds_for(env_name, dtype, reverse=True)
        _REV[key] = (spec, build(env_name, spec, dtype, B, V, uniform or all_kinds[0], seed, reverse=True, plain=st, kinds=all_kinds), acts)
    return _REV[key]


def reverse_cotangents(dtype, B, rows, OW, S, seed=5):
    """helpers_vjp.cotangents in values the number format represents"""
    from helpers_vjp import cotangents

    npdt = np.dtype(dtype).type
    g = cotangents(np.random.default_rng(seed), B, rows, OW, S)
    r = lambda a: a.astype(npdt).astype(np.float64)
    return r(g[0]), [r(x) for x in g[1]], [r(x) for x in g[2]]


def by_kind(tensors_got, tensors_want, kinds, keep=None):
    """{kind: largest |got - want| over that kind's environments and over the tensors, each relative to the tensor's largest
    magnitude over ALL the environments given (the existing rule: "of each tensor's largest magnitude")}.
    tensors: lists of arrays whose first axis is the environment; kinds [n] names per environment; keep [n] bool."""
    out = {}
    everyone = np.ones(len(kinds), dtype=bool) if keep is None else keep
    for k in sorted(set(kinds)):
        sel = (kinds == k) & everyone
        if not sel.any():
            continue
        worst = 0.0
        for g, w in zip(tensors_got, tensors_want):
            g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
            scale = float(np.max(np.abs(w[everyone]), initial=0.0))
            d = float(np.max(np.abs(g[sel] - w[sel]), initial=0.0))
            worst = max(worst, d / scale if scale > 0 else d)
        out[k] = worst
    return out


def spread_by_kind(up, down, want, kinds, keep=None):
    """by_kind of `up` against `down` on the magnitudes of `want`: how far the reference itself moves under one ulp"""
    out = {}
    everyone = np.ones(len(kinds), dtype=bool) if keep is None else keep
    for k in sorted(set(kinds)):
        sel = (kinds == k) & everyone
        worst = 0.0
        for u, d, w in zip(up, down, want):
            scale = float(np.max(np.abs(np.asarray(w)[everyone]), initial=0.0))
            diff = float(np.max(np.abs(np.asarray(u)[sel] - np.asarray(d)[sel]), initial=0.0))
            worst = max(worst, diff / scale if scale > 0 else diff)
        out[k] = worst
    return out


def bound_of(base, spread):
    """The bound of a comparison and the rule that set it: the existing one, or 16 x the reference's own spread under one ulp of
    the special values where that spread exceeds it (no implementation can be closer to the reference than the reference is to
    itself; 16 x is the margin the saturated-model tests use)"""
    return (base, "existing bound") if spread <= base else (16 * spread, "16 x the reference's spread under one ulp")


_TWIN_REF = {}


def twin_reference(env_name, deadtime, solver, semantics, dtype, V, sub, K=REV_K, uniform=None, kinds=None, last_only=False):
    """The twin on the SPECIAL environments of reverse_setup (the environments are independent, so the twin runs on them alone):
    dict(idx: their indices, kinds, groups: the cotangents [B, ...], want: (grad_actions, [grad leaves]) on idx, spread: {kind:
    by_kind of the gradients at the special leaves + 1 ulp against - 1 ulp}, keep: idx at least KINK_MARGIN from a kink, obs:
    the twin's forward observations on idx). last_only: cotangents on the last observation row and the last state alone (what
    one reverse-mode step takes). Computed once per form and shared."""
    from helpers_vjp import KINK_MARGIN, Twin, twin_grads

    key = (env_name, deadtime, solver, semantics, np.dtype(dtype).name, V, sub, K, uniform, tuple(kinds or ()), last_only)
    if key in _TWIN_REF:
        return _TWIN_REF[key]
    spec, built, acts = reverse_setup(env_name, deadtime, dtype, V, K, uniform, kinds)
    idx = np.flatnonzero(built["mask"])
    B, S = acts.shape[0], len(built["special"])
    O = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][2]
    grp = reverse_cotangents(dtype, B, K * sub + 1, O, S)
    if last_only:  # the cotangents of one vmap_step: the new observation and the new state
        grp[0][:, :-1] = 0.0
        grp = (grp[0], None, grp[2])
    sub_grp = (grp[0][idx], None if grp[1] is None else [g[idx] for g in grp[1]], [g[idx] for g in grp[2]])
    acts64 = acts[idx].astype(np.float64)

    def run(leaves):
        twin = Twin(env_name, spec, solver, semantics)
        (want,), kd, obs = twin_grads(twin, [v[idx].astype(np.float64) for v in leaves], acts64, spec["tau"], sub, [sub_grp], O)
        return want, kd, obs

    want, kd, obs = run(built["special"])
    angles = built["written"].copy()  # "the special angles move by one ulp": the angle leaves only
    angles[[j for j in range(S) if j not in ANGLE_STATES.get(env_name, [])]] = False
    up, _, _ = run(one_ulp(built["special"], angles, +1))
    down, _, _ = run(one_ulp(built["special"], angles, -1))
    kinds_idx = built["kind"][idx]
    flat = lambda w: [w[0]] + list(w[1])
    keep = np.ones(idx.size, dtype=bool) if kd is None else (kd.numpy() >= KINK_MARGIN)
    spread = spread_by_kind(flat(up), flat(down), flat(want), kinds_idx, keep)
    _TWIN_REF[key] = dict(idx=idx, kinds=kinds_idx, groups=grp, want=want, spread=spread, keep=keep, obs=obs, spec=spec, built=built, acts=acts)
    if len(_TWIN_REF) > 64:
        _TWIN_REF.pop(next(iter(_TWIN_REF)))
    return _TWIN_REF[key]


# ====================================================================== the closed loop's reverse mode
FB_SEED = REV_SEED  # the seed of the policy's inputs (helpers_feedback.feedback_inputs); the states are reverse_setup's


def feedback_reverse_subs(env_name):
    return (1,) if env_name == "pmsm" else (1, 2)


_FB_REF = {}


def feedback_twin_reference(env_name, deadtime, solver, dtype, sub, uniform, K=REV_K):
    """twin_reference for `vmap_sim_ahead_feedback_vjp`: the states of reverse_setup (V = 1, B = 326) under the full policy of
    helpers_feedback.feedback_inputs (per-environment gains, integral action, feedforward, clip), all five cotangents, the float64
    closed-loop twin (helpers_feedback_vjp.twin_run) on the SPECIAL environments alone. -> dict(idx, kinds, built, spec, inp: the
    inputs over all B in values the number format represents (st: the special states), group: the cotangents over all B, want:
    (first gradient, [the others]) on idx in the order state0 leaves, gain, integral gain, feedforward, integrator state, spread: the
    same one-ulp perturbation of the special angles as twin_reference's, pushed through twin_run, keep, obs: the twin's forward
    observations on idx). Computed once per form and shared."""
    import helpers_feedback as hf
    import helpers_feedback_vjp as hv
    from helpers_vjp import KINK_MARGIN

    key = (env_name, deadtime, solver, np.dtype(dtype).name, sub, uniform, K)
    if key in _FB_REF:
        return _FB_REF[key]
    npdt = np.dtype(dtype).type
    kinds = kinds_for(env_name, dtype, reverse=True)
    spec, built, _ = reverse_setup(env_name, deadtime, dtype, 1, K, uniform, kinds)
    B, S = built["mask"].shape[0], len(built["special"])
    idx = np.flatnonzero(built["mask"])
    r = lambda a: None if a is None else np.asarray(a).astype(npdt).astype(np.float64)
    raw = hf.feedback_inputs(env_name, spec, B, K, seed=FB_SEED)
    inp = dict(st=[v.astype(np.float64) for v in built["special"]], gain=r(raw["gain"]), igain=r(raw["igain"]), ff=r(raw["ff"]), z0=r(raw["z0"]),
               refs=None)
    O = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][2]
    A = oracle.ENV_DIMS[oracle.ENV_IDS[env_name]][1]
    full = hv.cotangent_groups(np.random.default_rng(5), B, K * sub + 1, O, S, K, A)[0]
    group = {k: ([r(x) for x in v] if isinstance(v, list) else r(v)) for k, v in full.items()}
    on = lambda v: [x[idx] for x in v] if isinstance(v, list) else v[idx]
    sub_group = {k: on(v) for k, v in group.items()}

    def run(leaves):
        part = dict(inp, st=[v[idx].astype(np.float64) for v in leaves], gain=inp["gain"][idx], igain=inp["igain"][idx], ff=inp["ff"][idx],
                    z0=inp["z0"][idx])
        twin, lv, out = hv.twin_run(env_name, spec, solver, part, K, sub)
        g = hv.twin_grads(lv, out, [sub_group], O)[0]
        kd = twin.kink_distance()
        return list(g["state0"]) + [g["gain"], g["igain"], g["ff"], g["z0"]], kd, out["obs"].detach().numpy()

    want, kd, obs = run(built["special"])
    angles = built["written"].copy()  # "the special angles move by one ulp": the angle leaves only
    angles[[j for j in range(S) if j not in ANGLE_STATES.get(env_name, [])]] = False
    up, _, _ = run(one_ulp(built["special"], angles, +1))
    down, _, _ = run(one_ulp(built["special"], angles, -1))
    kinds_idx = built["kind"][idx]
    keep = np.ones(idx.size, dtype=bool) if kd is None else (kd.numpy() >= KINK_MARGIN)
    _FB_REF[key] = dict(idx=idx, kinds=kinds_idx, built=built, spec=spec, inp=inp, group=group, want=(want[0], want[1:]),
                        spread=spread_by_kind(up, down, want, kinds_idx, keep), keep=keep, obs=obs)
    if len(_FB_REF) > 64:
        _FB_REF.pop(next(iter(_FB_REF)))
    return _FB_REF[key]
