"""The two key-stream kernels of csrc/refgen.hpp (``random_state_kernel``: ``vmap_init_state(keys)``; ``update_ref_kernel``:
``GymWrapper.update_ref``) on the paths tests/test_gpu_rng_oracle.py never launches or cannot see: the rare branches of the gamma
sampler with NO share of environments left out, per-environment and asymmetric state boxes, every state field as a control
column, hold ranges other than the three in use, batch tails, the saturated PMSM, and a reference stream with float work in it.
The reference is the oracle's restatement of jax.random (oracle/oracle_rng.inc); which keys take which path, and which few keys the
oracle itself decides within rounding (`fragile`, excluded where a batch is not built to avoid them), comes from the tracer of
tests/helpers_rng.py, whose conditions tests/test_rng_paths_host.py checks on the CPU. No tolerance is new: the currents and the
torque keep tests/test_gpu_rng_oracle.py's 256 eps on the 250 A scale, everything else is bit equality. ``-m gpu``; ``-s`` prints
the largest distance per path class."""
import functools

import numpy as np
import pytest
import torch

import oracle
import helpers_rng as hr
from exciting_environments_amd import _native
from helpers import NP_DTYPE, make_env

pytestmark = pytest.mark.gpu
ENV_NAMES = ["pendulum", "mass_spring_damper", "cartpole", "acrobot", "fluid_tank", "pmsm"]
DTYPES = [torch.float32, torch.float64]
CONTROL = {"pendulum": ["theta"], "mass_spring_damper": ["deflection", "velocity"], "cartpole": ["theta", "deflection"],
           "acrobot": ["theta_1", "omega_2"], "fluid_tank": ["height"], "pmsm": ["i_d", "i_q", "torque"]}
BALL_FIELDS = ("i_d", "i_q", "torque")  # what comes out of erf_inv / log / pow / sqrt; every other leaf is exact


# ---- launches ------------------------------------------------------------------------------------------------------------------------
def _dev(x, device):
    """A device copy of a host array (the shared references are read-only)"""
    return torch.from_numpy(np.array(x)).to(device)


def init_state(env, keys):
    """``env.vmap_init_state(keys)`` through excenv_random_state (asserted: the torch twin must not answer) -> (S arrays, key leaf)"""
    calls = []
    real = _native.random_state

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    _native.random_state = spy
    try:
        state = env.vmap_init_state(_dev(keys, env.device))
    finally:
        _native.random_state = real
    assert len(calls) == 1, "vmap_init_state(keys) did not launch excenv_random_state"
    assert state.PRNGKey.dtype == torch.int64
    return [getattr(state.physical_state, n).cpu().numpy() for n in env.STATE_FIELDS], state.PRNGKey.cpu().numpy()


def update_ref_both(env, idx, refs, keys, hold, lo, hi):
    """excenv_update_ref_to and excenv_update_ref on the same inputs -> [(references, keys, hold counters)] of the two as host
    arrays; the out-of-place launch must leave its inputs as they were"""
    B, dev = keys.shape[0], env.device
    p, _keep = env._props_for(env.env_properties, B)
    k_in, h_in = _dev(keys, dev), _dev(hold, dev)
    r_in = [_dev(r, dev) for r in refs]
    r_out = [torch.full_like(r, float("nan")) for r in r_in]
    k_out, h_out = torch.full_like(k_in, -1), torch.full_like(h_in, -99)
    _native.update_ref_to(env.ENV_ID, env.dtype, B, p, idx, r_in, k_in, h_in, r_out, k_out, h_out, lo, hi)
    r_ip, k_ip, h_ip = [r.clone() for r in r_in], k_in.clone(), h_in.clone()
    _native.update_ref(env.ENV_ID, env.dtype, B, p, idx, r_ip, k_ip, h_ip, lo, hi)
    torch.cuda.synchronize()
    assert np.array_equal(k_in.cpu().numpy(), keys) and np.array_equal(h_in.cpu().numpy(), hold)
    assert all(np.array_equal(t.cpu().numpy(), r) for t, r in zip(r_in, refs))
    host = lambda rr, kk, hh: ([t.cpu().numpy() for t in rr], kk.cpu().numpy(), hh.cpu().numpy())
    return [host(r_out, k_out, h_out), host(r_ip, k_ip, h_ip)]


def held_inputs(B, n, np_dtype, due, seed):
    """Hold counters that are 0 exactly where `due`, and n reference leaves to carry over"""
    rng = np.random.default_rng(seed)
    hold = np.where(due, 0, rng.integers(1, 4, B)).astype(np.int64)
    return hold, [rng.uniform(-1, 1, B).astype(np_dtype) for _ in range(n)]


def check_state(env_name, got, want, dtype, keep=None, label=""):
    """Every leaf of a drawn state: the PMSM's currents and torque within the tolerance wherever `keep`, the rest bit-equal everywhere"""
    tol = hr.ball_tolerance(NP_DTYPE[dtype])
    for j, n in enumerate(oracle.STATE_FIELDS[env_name]):
        if env_name == "pmsm" and n in BALL_FIELDS:
            d = np.abs(got[j].astype(np.float64) - want[j])
            d = d if keep is None else d[keep]
            assert np.isfinite(got[j]).all() and (d <= tol).all(), (label, n, float(d.max()), int((d > tol).sum()))
        else:
            assert np.array_equal(got[j], want[j]), (label, n)


def check_update(env_name, names, got, want, refs_in, due, dtype, keep=None, label=""):
    """One update_ref result against the oracle's: keys and hold counters exact, carried-over references bit-equal to their
    inputs, redrawn ones like check_state"""
    (g_refs, g_keys, g_hold), (w_refs, w_keys, w_hold) = got, want
    assert np.array_equal(g_keys, w_keys) and np.array_equal(g_hold, w_hold), label
    tol = hr.ball_tolerance(NP_DTYPE[dtype])
    sel = due if keep is None else due & keep
    for n, g, w, r in zip(names, g_refs, w_refs, refs_in):
        assert np.array_equal(g[~due], r[~due]), (label, n)
        if env_name == "pmsm" and n in BALL_FIELDS:
            d = np.abs(g.astype(np.float64) - w)[sel]
            assert np.isfinite(g).all() and (d <= tol).all(), (label, n, float(d.max(initial=0.0)), int((d > tol).sum()))
        else:
            assert np.array_equal(g, w), (label, n)


def by_class(got, want, cls, fields=(3, 4, 5)):
    return {c: max(float(np.abs(got[j].astype(np.float64) - want[j])[cls == c].max(initial=0.0)) for j in fields)
            for c in ("redo", "rounds", "plain")}


# ---- rare paths ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rare_reference(np_name):
    """The oracle on the rare batch, computed once per number format and shared read-only: dict(rb, want, want_leaf, due, hold,
    refs, idx, want_update)"""
    npdt = np.dtype(np_name).type
    rb = hr.rare_batch(npdt)
    B = rb["B"]
    from helpers import spec_of

    spec = spec_of("pmsm")
    props, keep = oracle.make_props("pmsm", spec["params"], spec["phys_norm"], spec["act_norm"], npdt, B)
    want, want_leaf = oracle.random_state("pmsm", rb["keys"], props, npdt)
    due = rb["rare"] | (np.arange(B) % 3 == 1)
    hold, refs = held_inputs(B, 3, npdt, due, seed=41)
    idx = [oracle.STATE_FIELDS["pmsm"].index(n) for n in CONTROL["pmsm"]]
    want_update = oracle.update_ref("pmsm", idx, refs, rb["keys"], hold, props, npdt, 10, 1000)
    for a in list(want) + [want_leaf] + list(want_update[0]) + list(want_update[1:]) + refs + [hold, due, rb["keys"], rb["plain_keys"]]:
        a.setflags(write=False)
    return dict(rb=rb, want=want, want_leaf=want_leaf, due=due, hold=hold, refs=refs, idx=idx, want_update=want_update)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rare_sampler_paths_match_the_oracle_in_every_environment(dtype):
    """Every redo key and every key of three or more rounds of a 2^17 pool in one batch of 1031, none of them fragile: keys and
    the uniform leaves exact, the currents and the torque within 256 eps x 250 in EVERY environment — through vmap_init_state and
    through both update_ref forms (due: every rare key and a third of the ordinary ones)."""
    ref = _rare_reference(np.dtype(NP_DTYPE[dtype]).name)
    rb, B = ref["rb"], ref["rb"]["B"]
    env, props, keep, spec = make_env("pmsm", B, dtype)
    got, leaf = init_state(env, rb["keys"])
    worst = by_class(got, ref["want"], rb["cls"])
    print(f"\n{np.dtype(NP_DTYPE[dtype]).name} random_state: largest distance {', '.join(f'{c} {v:.3e}' for c, v in worst.items())} "
          f"(bound {hr.ball_tolerance(NP_DTYPE[dtype]):.3e})")
    assert np.array_equal(leaf, ref["want_leaf"])
    check_state("pmsm", got, ref["want"], dtype, label="random_state")
    assert not np.any(got[0]) and not np.any(got[1])  # the voltage buffers start at zero
    for form, res in zip(("update_ref_to", "update_ref"), update_ref_both(env, ref["idx"], ref["refs"], rb["keys"], ref["hold"], 10, 1000)):
        d = {c: max(float(np.abs(g.astype(np.float64) - w)[(rb["cls"] == c) & ref["due"]].max(initial=0.0))
                    for g, w in zip(res[0], ref["want_update"][0])) for c in ("redo", "rounds", "plain")}
        print(f"{np.dtype(NP_DTYPE[dtype]).name} {form}: largest distance {', '.join(f'{c} {v:.3e}' for c, v in d.items())}")
        check_update("pmsm", CONTROL["pmsm"], res, ref["want_update"], ref["refs"], ref["due"], dtype, label=form)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_lane_in_the_rare_loops_does_not_disturb_its_wave(dtype):
    """The cold-path suite's rule (a): the same launches with an ordinary key in place of every rare one — every output of every
    other environment is bit-equal between the two launches."""
    ref = _rare_reference(np.dtype(NP_DTYPE[dtype]).name)
    rb, B = ref["rb"], ref["rb"]["B"]
    others = ~rb["rare"]
    assert others.sum() > B // 2 and np.array_equal(rb["keys"][others], rb["plain_keys"][others])
    env, props, keep, spec = make_env("pmsm", B, dtype)
    a, leaf_a = init_state(env, rb["keys"])
    b, leaf_b = init_state(env, rb["plain_keys"])
    assert np.array_equal(leaf_a[others], leaf_b[others])
    for j, n in enumerate(env.STATE_FIELDS):
        assert np.array_equal(a[j][others], b[j][others]), n
        if n in ("i_d", "i_q"):
            assert not np.array_equal(a[j][~others], b[j][~others])  # the replaced keys do draw something else
    two = [update_ref_both(env, ref["idx"], ref["refs"], k, ref["hold"], 10, 1000) for k in (rb["keys"], rb["plain_keys"])]
    for (ra, ka, ha), (rp, kp, hp) in zip(*two):
        assert np.array_equal(ka[others], kp[others]) and np.array_equal(ha[others], hp[others])
        for x, y in zip(ra, rp):
            assert np.array_equal(x[others], y[others])


# ---- per-environment, asymmetric boxes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_per_environment_asymmetric_boxes(env_name, dtype):
    """helpers_vjp.skewed_spec with three state bounds as [B] arrays (PMSM: bounds of i_d and i_q, so i_max differs per
    environment and each of the four mirror terms fires): the BATCHED property load, against the oracle with the same arrays"""
    B, npdt = 257, NP_DTYPE[dtype]
    keys, tr, seed = hr.plain_keys(npdt, B)
    keep = ~tr["fragile"]
    print(f"\n{env_name} {np.dtype(npdt).name}: keys of seed {seed}, {int((~keep).sum())} fragile key(s) excluded")
    assert (~keep).sum() <= 1
    spec, plan = hr.per_env_spec(env_name, B)
    env, props, _keep, _ = make_env(env_name, B, dtype, spec=spec)
    want, want_leaf = oracle.random_state(env_name, keys, props, npdt)
    got, leaf = init_state(env, keys)
    assert np.array_equal(leaf, want_leaf)
    check_state(env_name, got, want, dtype, keep=keep, label="random_state")
    names = CONTROL[env_name]
    idx = [env.STATE_FIELDS.index(n) for n in names]
    due = np.arange(B) % 3 != 1
    hold, refs = held_inputs(B, len(idx), npdt, due, seed=43)
    want_u = oracle.update_ref(env_name, idx, refs, keys, hold, props, npdt, 10, 1000)
    for form, res in zip(("update_ref_to", "update_ref"), update_ref_both(env, idx, refs, keys, hold, 10, 1000)):
        check_update(env_name, names, res, want_u, refs, due, dtype, keep=keep, label=form)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("env_name", ENV_NAMES)
def test_every_state_field_as_a_control_column(env_name, dtype):
    """control_idx = all S fields in a shuffled order (PMSM: 7 of EXCENV_MAX_CONTROL = 8): the select chain of update_ref_kernel
    hands each reference leaf its own field"""
    B, npdt = 257, NP_DTYPE[dtype]
    from helpers_vjp import skewed_spec

    keys, tr, seed = hr.plain_keys(npdt, B)
    keep = ~tr["fragile"]
    assert (~keep).sum() <= 1
    fields = oracle.STATE_FIELDS[env_name]
    rng = np.random.default_rng(len(fields))
    idx = [int(j) for j in rng.permutation(len(fields))]
    while len(idx) > 1 and idx == sorted(idx):
        idx = [int(j) for j in rng.permutation(len(fields))]
    assert sorted(idx) == list(range(len(fields))) and len(idx) <= oracle.MAX_CONTROL
    names = [fields[j] for j in idx]
    env, props, _keep, _ = make_env(env_name, B, dtype, spec=skewed_spec(env_name))
    due = np.arange(B) % 4 != 2
    hold, refs = held_inputs(B, len(idx), npdt, due, seed=47)
    want_u = oracle.update_ref(env_name, idx, refs, keys, hold, props, npdt, 10, 1000)
    state, _ = oracle.random_state(env_name, keys, props, npdt)
    for q, j in enumerate(idx):  # the oracle's leaf q is field idx[q] of its own state, and no two distinct fields coincide
        assert np.array_equal(want_u[0][q][due], state[j][due])
    for form, res in zip(("update_ref_to", "update_ref"), update_ref_both(env, idx, refs, keys, hold, 10, 1000)):
        check_update(env_name, names, res, want_u, refs, due, dtype, keep=keep, label=form)


# ---- hold ranges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_hold_ranges_on_the_device(dtype):
    """rng_randint (fp32: the int32 form) and rng_randint64 (fp64: the x64 form) with every environment due: an empty range, a
    reversed one, spans of 1, above 65536 and of 2^31 - 1, a negative lower bound — and ranges whose difference leaves int32, where
    the span is the unsigned difference like in the oracle (jax/_src/random.py _randint computes it in the unsigned type)."""
    B, npdt = 257, NP_DTYPE[dtype]
    env, props, _keep, spec = make_env("pendulum", B, dtype)
    keys = oracle.split(oracle.prng_key(611), B)
    hold = np.zeros(B, dtype=np.int64)
    refs = [np.zeros(B, dtype=npdt)]
    form = oracle.randint if dtype == torch.float32 else oracle.randint64
    _, leaf = oracle.random_state("pendulum", keys, props, npdt)
    sub = oracle.split(leaf)[:, 1]
    for lo, hi in hr.HOLD_RANGES + hr.WIDE_HOLD_RANGES:
        want = oracle.update_ref("pendulum", [0], refs, keys, hold, props, npdt, lo, hi)
        assert np.array_equal(want[2], form(sub, 1, lo, hi)[:, 0] - 1)  # the oracle's own two statements agree
        if hi > lo:
            assert want[2].min() >= lo - 1 and want[2].max() < hi - 1, (lo, hi)
        assert len(np.unique(want[2])) == 1 if hr.span_of(lo, hi) == 1 else len(np.unique(want[2])) >= 2
        for name, res in zip(("update_ref_to", "update_ref"), update_ref_both(env, [0], refs, keys, hold, lo, hi)):
            assert np.array_equal(res[2], want[2]), (name, lo, hi, res[2][:4], want[2][:4])
            assert np.array_equal(res[1], want[1]) and np.array_equal(res[0][0], want[0][0]), (name, lo, hi)


# ---- batch tails ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("env_name", ["pendulum", "pmsm"])
def test_batch_tails(env_name, B, dtype):
    npdt = NP_DTYPE[dtype]
    keys, tr, seed = hr.plain_keys(npdt, B, base=700)
    keep = ~tr["fragile"]
    assert (~keep).sum() <= 1
    env, props, _keep, spec = make_env(env_name, B, dtype)
    want, want_leaf = oracle.random_state(env_name, keys, props, npdt)
    got, leaf = init_state(env, keys)
    assert np.array_equal(leaf, want_leaf)
    check_state(env_name, got, want, dtype, keep=keep)
    names = CONTROL[env_name]
    idx = [env.STATE_FIELDS.index(n) for n in names]
    due = np.arange(B) % 3 != 1  # B = 1: the one environment is due
    hold, refs = held_inputs(B, len(idx), npdt, due, seed=53)
    want_u = oracle.update_ref(env_name, idx, refs, keys, hold, props, npdt, 3, 40)
    for form, res in zip(("update_ref_to", "update_ref"), update_ref_both(env, idx, refs, keys, hold, 3, 40)):
        check_update(env_name, names, res, want_u, refs, due, dtype, keep=keep, label=form)


# ---- the saturated PMSM --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_saturated_pmsm_draws_its_torque_from_the_tables(dtype):
    """random_state_kernel<PmsmSat> / update_ref_kernel<PmsmSat> against the oracle built with the same tables (oracle.make_props
    carries them: pmsm_torque reads the flux linkages out of the tables when they are set). Currents: the tolerance above. Torque:
    tests/test_gpu_saturated.py's bound for one table read (rtol = tol, atol = 200 tol; tol = 5e-5 in fp32, 1e-9 in fp64)."""
    from helpers_lut import make_saturated, saturating_lut

    B, npdt = 257, NP_DTYPE[dtype]
    keys, tr, seed = hr.plain_keys(npdt, B)
    keep = ~tr["fragile"]
    assert (~keep).sum() <= 1
    env, props, _keep, spec = make_saturated(B, dtype, "euler", saturating_lut(holes=False))
    want, want_leaf = oracle.random_state("pmsm", keys, props, npdt)
    from helpers import spec_of

    lin_props, _k2 = oracle.make_props("pmsm", spec_of("pmsm")["params"], spec["phys_norm"], spec["act_norm"], npdt, B)
    linear, _ = oracle.random_state("pmsm", keys, lin_props, npdt)
    assert np.abs(want[5] - linear[5]).max() > 1.0  # the tables do say something else than the linear model
    tol = 5e-5 if dtype == torch.float32 else 1e-9

    def check(got, ref, sel, label):
        for j in (3, 4):
            d = np.abs(got[j].astype(np.float64) - ref[j])[sel]
            assert (d <= hr.ball_tolerance(npdt)).all(), (label, j, float(d.max()))
        assert np.allclose(got[5][sel], ref[5][sel], rtol=tol, atol=200 * tol), (label, float(np.abs(got[5] - ref[5])[sel].max()))

    got, leaf = init_state(env, keys)
    assert np.array_equal(leaf, want_leaf)
    for j in (0, 1, 2, 6):
        assert np.array_equal(got[j], want[j])
    check(got, want, keep, "random_state")
    idx = [3, 4, 5]
    due = np.arange(B) % 3 != 1
    hold, refs = held_inputs(B, 3, npdt, due, seed=59)
    want_u = oracle.update_ref("pmsm", idx, refs, keys, hold, props, npdt, 10, 1000)
    for form, res in zip(("update_ref_to", "update_ref"), update_ref_both(env, idx, refs, keys, hold, 10, 1000)):
        assert np.array_equal(res[1], want_u[1]) and np.array_equal(res[2], want_u[2]), form
        for g, r in zip(res[0], refs):
            assert np.array_equal(g[~due], r[~due]), form
        check({3 + q: g for q, g in enumerate(res[0])}, {3 + q: w for q, w in enumerate(want_u[0])}, due & keep, form)


# ---- a stream with float work in it ---------------------------------------------------------------------------------------------------
def test_pmsm_reference_stream_keeps_its_keys_whatever_the_floats_do():
    """GymWrapper over the PMSM in fp32, references i_d and i_q, hold range (1, 4), 64 steps from one key: keys and hold counters
    equal the oracle's update_ref applied 64 times, exactly (integer work must not depend on a float); every reference whose latest
    draw was not fragile meets the tolerance at every step."""
    from exciting_environments_amd import GymWrapper

    B, steps, lo, hi = 256, 64, 1, 4
    dtype, npdt = torch.float32, np.float32
    env, props, _keep, spec = make_env("pmsm", B, dtype)
    names, idx = ["i_d", "i_q"], [3, 4]

    def oracle_stream(seed):
        """The oracle's stream from split(PRNGKey(seed), B): reset draws for everyone (and does not count down), then one update_ref
        per step -> (keys, [(references, keys, hold counters, who drew at this step, the keys drawn from)], fragile per draw)"""
        keys = oracle.split(oracle.prng_key(seed), B)
        refs, k, h = oracle.update_ref("pmsm", idx, [np.zeros(B, dtype=npdt)] * 2, keys, np.zeros(B, dtype=np.int64), props, npdt, lo, hi)
        trail = [(refs, k, h + 1, np.ones(B, dtype=bool), keys)]
        for _ in range(steps):
            refs, k_prev, h_prev = trail[-1][:3]
            refs, k, h = oracle.update_ref("pmsm", idx, refs, k_prev, h_prev, props, npdt, lo, hi)
            trail.append((refs, k, h, h_prev == 0, k_prev))
        return keys, trail, hr.trace_ball(np.concatenate([t[4][t[3]] for t in trail]), npdt)["fragile"]

    # the share of fragile draws is a property of the oracle's stream, known before anything is launched: the first seed within the
    # cap (one seed in ten draws a third fragile key out of 8 000: the pool's share is 1.3e-4)
    for seed in range(19, 27):
        keys, trail, fragile = oracle_stream(seed)
        cap = 2e-4 * fragile.shape[0] + 1
        print(f"\nseed {seed}: {fragile.shape[0]} draws over {steps} steps, {int(fragile.sum())} fragile (cap {cap:.1f})")
        if fragile.sum() <= cap:
            break
    drawn = fragile
    assert drawn.shape[0] > 10 * B and fragile.sum() <= cap
    gw = GymWrapper(env=env, control_state=names, ref_params={"hold_steps_min": lo, "hold_steps_max": hi})
    gw.reset(rng_ref=_dev(keys, env.device))
    act = torch.zeros((B, 2), dtype=dtype, device=env.device)
    ok, at, worst = np.ones(B, dtype=bool), 0, 0.0
    for t, (w_refs, w_keys, w_hold, due, _) in enumerate(trail):
        if t:
            gw.step(act)
        ok[due] = ~fragile[at:at + int(due.sum())]
        at += int(due.sum())
        assert np.array_equal(gw.state.PRNGKey.cpu().numpy(), w_keys), t
        assert np.array_equal(gw.reference_hold_steps.reshape(B).cpu().numpy(), w_hold), t
        for n, w in zip(names, w_refs):
            d = np.abs(getattr(gw.state.reference, n).cpu().numpy().astype(np.float64) - w)[ok]
            worst = max(worst, float(d.max(initial=0.0)))
            assert (d <= hr.ball_tolerance(npdt)).all(), (t, n, float(d.max()))
    print(f"largest distance of a non-fragile reference {worst:.3e} (bound {hr.ball_tolerance(npdt):.3e})")
    assert at == drawn.shape[0] and len(np.unique(trail[-1][2])) >= 2 and not np.array_equal(trail[-1][1], trail[1][1])
