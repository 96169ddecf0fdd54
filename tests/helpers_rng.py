"""A path tracer for the key-stream kernels' only data-dependent control flow: the Marsaglia-Tsang rejection loops behind the PMSM's
random currents (csrc/refgen.hpp rng_gamma_one; oracle/oracle_rng.inc:70-108), shared by tests/test_rng_paths_host.py and
tests/test_gpu_rng_paths.py. Nothing here needs a GPU.

``init_state_from_key`` of the PMSM draws its currents through ``ball(key, 2)``: two ``gamma(1/2)`` samples, each an outer rejection
loop (accept when ``U < 1 - 0.0331 X^2`` or ``log U < X/2 + d((1 - V) + log V)``) around an inner loop that redraws the normal
while ``v = 1 + x c <= 0``. The tracer restates that key tree in numpy on top of the oracle's primitives (``oracle.split``,
``oracle.normal``, ``oracle.uniform``): the drawn values are carried in the working precision with the oracle's own operation
order (one rounding per operation on both sides: the same bits), the two sides of every comparison are evaluated in float64. Per
key it reports the outer rounds of each gamma draw, the inner redraws, and the smallest DECISION MARGIN it met: how far, relative
to the magnitude of the terms compared, a comparison was from going the other way. A key is FRAGILE when that margin is below
``256 eps`` — the value tolerance tests/test_gpu_rng_oracle.py already grants the device's math library against the oracle's
(``_ball_tolerance``): there a device logarithm that differs by a few ulp may decide differently and draw another sample, and
neither sample is wrong. Everything else about the state is continuous in the drawn values (square root, power, the mirror terms)
or compares bit-exact uniforms (the Rademacher sign), so a non-fragile key has no excuse.

The thresholds and counts asserted in tests/test_rng_paths_host.py are conditions on the oracle's outputs; nothing here looks at a
device result."""
import numpy as np

import oracle

POOL = 1 << 17
FRAGILE_EPS = 256       # tests/test_gpu_rng_oracle.py _ball_tolerance
CURRENT_SCALE = 250.0   # the same file's scale of the currents and the torque
MIN_REDO, MIN_ROUNDS3 = 64, 64
WAVE = 64
SQUEEZE = 0.0331


def fragile_below(dtype):
    return FRAGILE_EPS * float(np.finfo(np.dtype(dtype)).eps)


def ball_tolerance(dtype):
    """The absolute bound of a current or a torque: 256 eps of the number format on the 250 A scale"""
    return fragile_below(dtype) * CURRENT_SCALE


def _rel(a, b, *more):
    """|a - b| relative to the largest magnitude among the terms given (1 where all of them are 0)"""
    scale = np.maximum(np.abs(a), np.abs(b))
    for t in more:
        scale = np.maximum(scale, np.abs(t))
    return np.abs(a - b) / np.where(scale > 0, scale, 1.0)


def trace_gamma(keys, dtype):
    """``_gamma_one(key, 1/2)`` for every key of [m, 2] -> dict(rounds [m]: executions of the outer body (>= 1), redo [m]: inner
    redraws (v <= 0), margin [m]: the smallest decision margin, V, gamma [m]: the accepted V and the sample rebuilt from it)"""
    dt = np.dtype(dtype).type
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    m = keys.shape[0]
    one, third = dt(1), dt(1.0 / 3.0)
    alpha_orig = dt(0.5)
    d = (alpha_orig + one) - third
    c = third / np.sqrt(d)
    d64, c64 = float(d), float(c)
    sp = oracle.split(keys, 2)
    k, subkey = sp[:, 0].copy(), sp[:, 1]
    X, V, U = np.zeros(m, dtype=dt), np.ones(m, dtype=dt), np.full(m, 2, dtype=dt)
    rounds, redo = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    margin = np.full(m, np.inf)
    active = np.arange(m)
    first = True
    while active.size:
        a = active
        x64, v64, u64 = X[a].astype(np.float64), V[a].astype(np.float64), U[a].astype(np.float64)
        rhs_a = 1.0 - SQUEEZE * (x64 * x64)
        term_a = u64 >= rhs_a
        m_a = _rel(u64, rhs_a)
        log_u, t1, t2, t3 = np.log(u64), x64 * 0.5, d64 * (1.0 - v64), d64 * np.log(v64)
        rhs_b = t1 + (t2 + t3)
        term_b = log_u >= rhs_b
        m_b = _rel(log_u, rhs_b, t1, t2, t3)
        again = term_a & term_b
        # `again` true: either term going the other way ends the loop. False: every false term has to turn (and no true one)
        m_dec = np.where(again, np.minimum(m_a, m_b), np.where(term_a, m_b, np.where(term_b, m_a, np.maximum(m_a, m_b))))
        if not first:  # the first test compares constants (U = 2, X = 0, V = 1)
            margin[a] = np.minimum(margin[a], m_dec)
        cont = a[again]
        if not cont.size:
            break
        sp3 = oracle.split(k[cont], 3)
        k_next, x_key, u_key = sp3[:, 0], sp3[:, 1].copy(), sp3[:, 2]
        x, v = np.zeros(cont.size, dtype=dt), np.full(cont.size, -1, dtype=dt)
        need = np.arange(cont.size)
        while need.size:
            s2 = oracle.split(x_key[need], 2)
            xn = oracle.normal(s2[:, 1], dt)
            prod = xn * c
            vn = one + prod
            x[need], v[need], x_key[need] = xn, vn, s2[:, 0]
            margin[cont[need]] = np.minimum(margin[cont[need]], _rel(np.ones(need.size), -(xn.astype(np.float64) * c64)))
            bad = vn <= 0
            redo[cont[need[bad]]] += 1
            need = need[bad]
        X[cont], V[cont] = x * x, (v * v) * v
        U[cont] = oracle.uniform(u_key, 1, dt)[:, 0]
        k[cont] = k_next
        rounds[cont] += 1
        active = cont
        first = False
    samples = one - oracle.uniform(subkey, 1, dt)[:, 0]
    boost = np.power(samples, one / alpha_orig)
    return dict(rounds=rounds, redo=redo, margin=margin, V=V, gamma=(d * V) * boost)


def ball_key(keys):
    """The key ``init_state_from_key`` of the PMSM passes to ``ball``: split(split(key)[0])[1]"""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    return oracle.split(oracle.split(keys, 2)[:, 0], 2)[:, 1]


def trace_ball(keys, dtype):
    """The PMSM's ``init_state_from_key`` -> ``ball`` -> two ``gamma(1/2)`` for environment keys [n, 2] -> dict(rounds [n, 2], redo
    [n, 2], margin [n], fragile [n], gamma_key [n, 2]: the key whose ``gamma(key, 1/2, (2,))`` the two draws are, ball_key [n, 2],
    gamma [n, 2], disc [n, 2]: the samples and the disc point rebuilt from the traced path)"""
    dt = np.dtype(dtype).type
    bk = ball_key(keys)
    n = bk.shape[0]
    sp = oracle.split(bk, 2)
    k1, k2 = sp[:, 0], sp[:, 1]
    sp1 = oracle.split(k1, 2)
    kg, kr = sp1[:, 0], sp1[:, 1]
    tr = trace_gamma(oracle.split(kg, 2).reshape(2 * n, 2), dt)
    rounds, redo, gam = tr["rounds"].reshape(n, 2), tr["redo"].reshape(n, 2), tr["gamma"].reshape(n, 2)
    margin = tr["margin"].reshape(n, 2).min(axis=1)
    sign = np.where(oracle.uniform(kr, 2, dt) < dt(0.5), dt(1), dt(-1)).astype(dt)
    g = sign * np.sqrt(gam)
    e = oracle.exponential(k2, dt)
    nrm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + e)
    return dict(rounds=rounds, redo=redo, margin=margin, fragile=margin < fragile_below(dt), gamma_key=kg, ball_key=bk, gamma=gam,
                disc=g / nrm[:, None])


def classify(tr):
    """[n] names: 'redo' (an inner redraw), 'rounds' (a gamma draw of three or more outer rounds, no redraw), 'plain'"""
    out = np.array(["plain"] * tr["margin"].shape[0], dtype=object)
    out[tr["rounds"].max(axis=1) >= 3] = "rounds"
    out[tr["redo"].sum(axis=1) > 0] = "redo"
    return out


_POOL, _RARE, _PLAIN = {}, {}, {}


def pool(dtype, seed):
    """(keys [2^17, 2], trace_ball of them), traced once per number format and seed"""
    key = (np.dtype(dtype).name, seed)
    if key not in _POOL:
        if len(_POOL) >= 4:
            _POOL.pop(next(iter(_POOL)))
        keys = oracle.split(oracle.prng_key(seed), POOL)
        _POOL[key] = (keys, trace_ball(keys, dtype))
    return _POOL[key]


def pool_counts(tr):
    cls = classify(tr)
    return dict(redo=int((cls == "redo").sum()), rounds3=int((tr["rounds"].max(axis=1) >= 3).sum()),
                rounds4=int((tr["rounds"].max(axis=1) >= 4).sum()), rounds2=int((tr["rounds"].max(axis=1) >= 2).sum()),
                fragile=int(tr["fragile"].sum()), fragile_share=float(tr["fragile"].mean()))


def rare_slots(B, n_rare):
    """The lane pattern of helpers_cold.special_envs for `n_rare` rare keys (wave = environment // 64): environment 0 alone in wave
    0; one in the middle of wave 1, alone; none in wave 2; every environment of wave 3 (64 redo keys); environment B - 1 alone in
    the ragged last wave; the others spread evenly over the waves in between. -> (uniform [64], single [3], spread [n_rare - 67])"""
    waves = -(-B // WAVE)
    assert waves >= 6 and (B - 1) // WAVE == waves - 1 and n_rare >= WAVE + 3, (B, n_rare)
    uniform = np.arange(3 * WAVE, 4 * WAVE)
    single = np.array([0, WAVE + 32, B - 1])
    room = np.arange(4 * WAVE, (waves - 1) * WAVE)
    rest = n_rare - WAVE - 3
    assert rest <= room.size // 2, (rest, room.size)  # at most every other lane: the waves stay mixed
    spread = room[(np.arange(rest) * room.size) // max(rest, 1)]
    return uniform, single, spread


def rare_batch(dtype, B=1031):
    """The batch of the rare-path tests -> dict(keys [B, 2]; plain_keys [B, 2]: the same with an ordinary key in place of every rare
    one; rare [B] bool; cls [B]: classify(); rounds, redo [B, 2]; margin [B]; seed; pool: pool_counts of the pool drawn from).
    The pool is ``split(PRNGKey(seed), 2^17)`` of the first seed that holds >= 64 non-fragile redo keys, >= 64 non-fragile keys of
    three or more rounds and one of four or more; fragile keys are dropped; every rare key is in the batch."""
    key = (np.dtype(dtype).name, B)
    if key in _RARE:
        return _RARE[key]
    for seed in range(16):
        keys, tr = pool(dtype, seed)
        ok = ~tr["fragile"]
        cls = classify(tr)
        redo_i, rounds_i, plain_i = (np.flatnonzero(ok & (cls == c)) for c in ("redo", "rounds", "plain"))
        if redo_i.size >= MIN_REDO and rounds_i.size >= MIN_ROUNDS3 and (tr["rounds"][ok].max(axis=1) >= 4).any():
            break
    else:
        raise AssertionError("no seed below 16 gives the rare-path counts")
    n_rare = redo_i.size + rounds_i.size
    uniform, single, spread = rare_slots(B, n_rare)
    # the four-round key goes to environment 0, redo keys to the uniform wave, to the wave-1 slot and to the tail
    deep = rounds_i[np.argmax(tr["rounds"][rounds_i].max(axis=1))]
    rest = np.concatenate([redo_i[WAVE + 2:], rounds_i[rounds_i != deep]])
    rest = rest[np.random.default_rng(seed).permutation(rest.size)]
    idx = np.full(B, -1, dtype=np.int64)
    idx[uniform] = redo_i[:WAVE]
    idx[single] = [deep, redo_i[WAVE], redo_i[WAVE + 1]]
    idx[spread] = rest
    rare = idx >= 0
    need = int((~rare).sum())
    assert plain_i.size >= need + B
    idx[~rare] = plain_i[:need]
    plain_idx = idx.copy()
    plain_idx[rare] = plain_i[need:need + int(rare.sum())]
    out = dict(keys=keys[idx].copy(), plain_keys=keys[plain_idx].copy(), rare=rare, cls=cls[idx], rounds=tr["rounds"][idx],
               redo=tr["redo"][idx], margin=tr["margin"][idx], seed=seed, pool=pool_counts(tr), B=B)
    assert int(rare.sum()) == n_rare and not tr["fragile"][idx].any() and not tr["fragile"][plain_idx].any()
    _RARE[key] = out
    return out


def wave_kinds(rare):
    """Per wave of 64 environments: 'clean', 'mixed' or 'uniform'"""
    out = []
    for w in range(-(-rare.size // WAVE)):
        part = rare[w * WAVE:(w + 1) * WAVE]
        out.append("uniform" if part.all() else ("mixed" if part.any() else "clean"))
    return out


def plain_keys(dtype, B, first_seeds=8, base=500):
    """(keys [B, 2] = split(PRNGKey(seed), B), trace_ball of them, seed): the first of a few seeds whose batch holds no fragile key,
    else the one with the fewest. Chosen on the CPU from the oracle's path alone."""
    key = (np.dtype(dtype).name, B, first_seeds, base)
    if key not in _PLAIN:
        best = None
        for seed in range(base, base + first_seeds):
            keys = oracle.split(oracle.prng_key(seed), B)
            tr = trace_ball(keys, dtype)
            n = int(tr["fragile"].sum())
            if best is None or n < best[0]:
                best = (n, keys, tr, seed)
            if n == 0:
                break
        _PLAIN[key] = best[1:]
    return _PLAIN[key]


# ---- per-environment, asymmetric boxes ---------------------------------------------------------------------------------------------
PER_ENV_SEED = 31
# PMSM: (field, which bound, the range of the per-environment factor on helpers_vjp.skewed_spec's bound). i_d's upper bound stays the
# skewed scalar (12.5 A): the largest magnitude i_max is then the lower bound of i_d, the lower or the upper bound of i_q, by environment
PMSM_PER_ENV = (("i_d", 0, (0.25, 1.25)), ("i_q", 0, (0.25, 1.25)), ("i_q", 1, (0.3, 1.7)))
GENERIC_FACTOR = (0.7, 1.3)


def per_env_spec(env_name, B, seed=PER_ENV_SEED):
    """helpers_vjp.skewed_spec with three state bounds (the tank has two) as [B] arrays -> (spec, [(field, bound)])"""
    from helpers_vjp import skewed_spec

    spec = skewed_spec(env_name)
    rng = np.random.default_rng(seed)
    fields = oracle.STATE_FIELDS[env_name]
    if env_name == "pmsm":
        plan = PMSM_PER_ENV
    else:
        plan = [(fields[0], 0, GENERIC_FACTOR), (fields[0], 1, GENERIC_FACTOR), (fields[-1], 1, GENERIC_FACTOR)]
        plan = list(dict.fromkeys(plan))  # one field: its two bounds
    for name, side, (f_lo, f_hi) in plan:
        box = list(spec["phys_norm"][name])
        box[side] = float(box[side]) * rng.uniform(f_lo, f_hi, B)
        spec["phys_norm"][name] = tuple(box)
    return spec, [(n, s) for n, s, _ in plan]


def pmsm_mirror_terms(keys, spec, dtype):
    """The oracle's disc point pushed through the current box in the working precision with init_state_from_key's operation order ->
    dict(fired [4, B]: i_d above its upper bound, below its lower one, i_q likewise; i_d, i_q [B]; bounds [4, B]: |i_d min|,
    |i_d max|, |i_q min|, |i_q max|; i_max [B])"""
    dt = np.dtype(dtype).type
    B = np.asarray(keys).reshape(-1, 2).shape[0]
    get = lambda name, side: np.broadcast_to(np.asarray(spec["phys_norm"][name][side], dtype=np.float64), (B,)).astype(dt)
    d_lo, d_hi, q_lo, q_hi = get("i_d", 0), get("i_d", 1), get("i_q", 0), get("i_q", 1)
    bounds = np.stack([np.abs(d_lo), np.abs(d_hi), np.abs(q_lo), np.abs(q_hi)])
    i_max = bounds.max(axis=0)
    disc = oracle.ball2(ball_key(keys), dt)
    xd, xq = disc[:, 0] * i_max, disc[:, 1] * i_max
    relu = lambda x: np.where(x > 0, x, dt(0)).astype(dt)
    i_d = xd - dt(2) * relu(xd - d_hi) + dt(2) * relu(-xd + d_lo)
    i_q = xq - dt(2) * relu(xq - q_hi) + dt(2) * relu(-xq + q_lo)
    fired = np.stack([xd - d_hi > 0, -xd + d_lo > 0, xq - q_hi > 0, -xq + q_lo > 0])
    return dict(fired=fired, i_d=i_d, i_q=i_q, bounds=bounds, i_max=i_max)


# ---- hold ranges ---------------------------------------------------------------------------------------------------------------------
INT32_MAX = (1 << 31) - 1
HOLD_RANGES = [(5, 5), (7, 3), (0, 1), (1, 2), (1, 65537), (1, 1 << 20), (-20, 40), (0, INT32_MAX)]
# hi - lo leaves int32: no caller can sensibly ask for these, but the span is defined (uint32 wrap-around, jax/_src/random.py _randint)
WIDE_HOLD_RANGES = [(-20, INT32_MAX), (-INT32_MAX - 1, INT32_MAX), (-(1 << 30), 1 << 30)]


def span_of(lo, hi):
    return 1 if hi <= lo else hi - lo
