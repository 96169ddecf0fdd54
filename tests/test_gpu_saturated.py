"""PMSM saturated (LUT) model on the GPU: HIP kernels vs the CPU oracle on a saturating machine with
NaN holes in the tables, and vs the linear-model kernels when the tables encode the linear motor. ``-m gpu``."""
import numpy as np
import pytest
import torch

import oracle
from helpers import NP_DTYPE, random_state, spec_of, to_state
from helpers_lut import linear_lut, make_saturated, saturating_lut, sew_shaped_lut

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", ["euler", "rk4", "tsit5"])
def test_saturated_step_and_sim_ahead_match_oracle(solver, dtype):
    # the synthetic machine is Euler-unstable at these speeds (errors double every few steps): fp32 is compared on a short
    # horizon, fp64 on the long one (kernel and oracle agree to 1e-12 there, so the arithmetic is the same)
    B, K = 2048, (48 if dtype == torch.float64 else 10)
    env, props, keep, spec = make_saturated(B, dtype, solver, saturating_lut())
    st = random_state("pmsm", B, NP_DTYPE[dtype], spec, seed=401)
    st[3][::5] = -400.0  # beyond the table: constant extrapolation through the padded edge
    rng = np.random.default_rng(402)
    acts = rng.uniform(-1, 1, (B, K, 2)).astype(NP_DTYPE[dtype])
    tol = 1e-9 if dtype == torch.float64 else 5e-5
    obs, new = env.vmap_step(to_state(env, st), torch.as_tensor(acts[:, 0], device=env.device))
    o_ref, s_ref = oracle.step("pmsm", solver, st, acts[:, 0], props, spec["tau"])
    assert np.allclose(obs.cpu().numpy(), o_ref, rtol=tol, atol=tol)
    assert np.allclose(new.physical_state.torque.cpu().numpy(), s_ref[5], rtol=tol, atol=tol * 200)
    for sem, osem in (("step", oracle.SEM_STEP), ("ahead", oracle.SEM_AHEAD)):
        env.sim_ahead_semantics = sem
        a_dev = env.new_actions_buffer(K)
        a_dev.copy_(torch.as_tensor(acts, device=env.device))
        o, s, l = env.vmap_sim_ahead(to_state(env, st), a_dev, env.tau, env.tau)
        o_ref, s_ref, l_ref = oracle.sim_ahead("pmsm", solver, st, acts, props, spec["tau"], semantics=osem)
        assert np.allclose(o.cpu().numpy(), o_ref, rtol=tol, atol=tol), (sem, float(np.abs(o.cpu().numpy() - o_ref).max()))
        assert np.allclose(s.physical_state.i_q.cpu().numpy(), s_ref[4], rtol=tol, atol=tol * 250)


def test_linear_tables_reproduce_the_linear_kernels():
    """Tables that encode the linear BRUSA motor: the saturated kernels agree with the linear-model kernels."""
    from exciting_environments_amd import EnvironmentRegistry, MotorVariant

    B, K = 1024, 64
    sp = MotorVariant.BRUSA.get_params().static_params
    lut = linear_lut(sp["l_d"], sp["l_q"], sp["psi_p"], i_d_range=(-2000, 2000), i_q_range=(-2000, 2000), n_d=81, n_q=81)
    env_s, props, keep, spec = make_saturated(B, torch.float64, "tsit5", lut)
    import exciting_environments_amd as ex
    env_l = EnvironmentRegistry.PMSM.make(batch_size=B, motor_variant=MotorVariant.BRUSA, solver=ex.Tsit5(), dtype=torch.float64, device="cuda")
    st = random_state("pmsm", B, np.float64, spec, seed=411)
    acts = torch.as_tensor(np.random.default_rng(412).uniform(-1, 1, (B, K, 2)), device="cuda")
    o_s, s_s, _ = env_s.vmap_sim_ahead(to_state(env_s, st), acts, env_s.tau, env_s.tau)
    o_l, s_l, _ = env_l.vmap_sim_ahead(to_state(env_l, st), acts, env_l.tau, env_l.tau)
    assert torch.allclose(o_s, o_l, rtol=1e-9, atol=1e-9)
    assert torch.allclose(s_s.physical_state.torque, s_l.physical_state.torque, rtol=1e-9, atol=1e-7)


def test_saturated_gym_step_and_layouts():
    B, K = 1024, 9
    env, props, keep, spec = make_saturated(B, torch.float32, "euler", saturating_lut(), control_state=["i_d", "i_q", "torque"])
    st = random_state("pmsm", B, np.float32, spec, seed=421)
    rng = np.random.default_rng(422)
    refs = {"i_d": rng.uniform(-200, -20, B).astype(np.float32), "i_q": rng.uniform(-200, 200, B).astype(np.float32),
            "torque": rng.uniform(-150, 150, B).astype(np.float32)}
    act = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
    state = to_state(env, st, reference=refs)
    obs, reward, term, trunc, new = env.vmap_gym_step(state, torch.as_tensor(act, device=env.device))
    o_ref, s_ref, r_ref, te_ref, tr_ref = oracle.gym_step("pmsm", "euler", st, act, props, spec["tau"],
                                                          control=[(n, refs[n]) for n in ("i_d", "i_q", "torque")])
    assert np.allclose(obs.cpu().numpy(), o_ref, rtol=2e-5, atol=2e-5) and np.allclose(reward.cpu().numpy(), r_ref, rtol=2e-5, atol=2e-5)
    assert np.array_equal(term.cpu().numpy(), te_ref) and np.array_equal(trunc.cpu().numpy(), tr_ref)
    acts = torch.as_tensor(rng.uniform(-1, 1, (B, K, 2)).astype(np.float32), device=env.device)
    env.traj_layout = "lane_major"
    o1, _, l1 = env.vmap_sim_ahead(state, acts, env.tau, env.tau)
    env.traj_layout = "env_major"
    o2, _, l2 = env.vmap_sim_ahead(state, acts, env.tau, env.tau)
    assert torch.equal(o1, o2) and torch.equal(l1.physical_state.i_d, l2.physical_state.i_d)


def test_non_uniform_grid_takes_the_exact_search_path():
    """The in-kernel cell search guesses arithmetically (linspace grids) and corrects against the stored grid; a strongly
    non-uniform grid must still give searchsorted's cell (binary-search fallback)."""
    import exciting_environments_amd as ex
    from exciting_environments_amd import EnvironmentRegistry, MotorVariant, prepare_pmsm_lut

    B = 4096
    lut = saturating_lut(holes=False)
    gd, gq, tab = prepare_pmsm_lut(lut)
    gd2 = np.sign(gd) * (np.abs(gd) / np.abs(gd).max()) ** 3 * np.abs(gd).max()  # cubic spacing, monotone
    gq2 = np.sign(gq) * (np.abs(gq) / np.abs(gq).max()) ** 3 * np.abs(gq).max()
    env = EnvironmentRegistry.PMSM.make(batch_size=B, saturated=True, motor_variant=MotorVariant.BRUSA, pmsm_lut=lut,
                                        dtype=torch.float64, device="cuda")
    env._lut_host = (gd2, gq2, tab)
    env._packed_props = None
    ep = env.env_properties
    params = {n: getattr(ep.static_params, n) for n in env.PARAM_FIELDS}
    pn = {n: (getattr(ep.physical_normalizations, n).min, getattr(ep.physical_normalizations, n).max) for n in env.STATE_FIELDS}
    an = {n: (getattr(ep.action_normalizations, n).min, getattr(ep.action_normalizations, n).max) for n in env.ACTION_FIELDS}
    props, keep = oracle.make_props("pmsm", params, pn, an, np.float64, B, pmsm_lut=(gd2, gq2, tab))
    spec = dict(params=params, phys_norm=pn, act_norm=an, tau=env.tau)
    st = random_state("pmsm", B, np.float64, spec, seed=431)
    st[3][:64] = gd2[np.arange(64) % gd2.size]  # exactly on grid nodes: side="left" semantics
    act = np.random.default_rng(432).uniform(-1, 1, (B, 2))
    obs, new = env.vmap_step(to_state(env, st), torch.as_tensor(act, device=env.device))
    o_ref, s_ref = oracle.step("pmsm", "euler", st, act, props, spec["tau"])
    assert np.allclose(obs.cpu().numpy(), o_ref, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sew_shaped_tables_with_circular_nan_region(dtype):
    """The grid and NaN geometry of the reference's SEW file (33 x 18 tables, i_d in [-16, 1] A, everything outside the
    current-limit circle NaN; values synthetic): prepare_pmsm_lut -> (20, 35) padded grids staged in LDS, kernels vs the
    oracle on states inside the circle, on its rim (cells whose corners were NaN-filled) and far outside (constant
    extrapolation), step and both trajectory semantics. fp32 is held to a short horizon and a looser bound: with the SEW
    voltage range (+-367 V) against ~2 mH one Euler step moves the currents by more than the table's whole range, so fp32
    rounding of the voltage path alone separates fp32 from fp64 by 2e-5 after one step and 5e-4 after eight (measured with
    the oracle); fp64 keeps the strict bound over 40 steps."""
    B, K = 2048, (40 if dtype == torch.float64 else 3)
    env, props, keep, spec = make_saturated(B, dtype, "euler", sew_shaped_lut(), variant="SEW")
    npdt = NP_DTYPE[dtype]
    rng = np.random.default_rng(441)
    ang, rad = rng.uniform(0, 2 * np.pi, B), np.concatenate([rng.uniform(0, 14, B // 2), rng.uniform(14, 17, B // 4), rng.uniform(17, 40, B - B // 2 - B // 4)])
    st = [np.zeros(B, npdt), np.zeros(B, npdt), rng.uniform(-3, 3, B).astype(npdt), (-np.abs(rad * np.cos(ang))).astype(npdt),
          (rad * np.sin(ang)).astype(npdt), np.zeros(B, npdt), rng.uniform(0, 300, B).astype(npdt)]
    acts = rng.uniform(-1, 1, (B, K, 2)).astype(npdt)
    tol = 1e-9 if dtype == torch.float64 else 2e-4
    obs, new = env.vmap_step(to_state(env, st), torch.as_tensor(acts[:, 0], device=env.device))
    o_ref, s_ref = oracle.step("pmsm", "euler", st, acts[:, 0], props, spec["tau"])
    assert np.isfinite(o_ref).all() and np.allclose(obs.cpu().numpy(), o_ref, rtol=tol, atol=tol)
    for sem, osem in (("step", oracle.SEM_STEP), ("ahead", oracle.SEM_AHEAD)):
        env.sim_ahead_semantics = sem
        for layout in ("lane_major", "env_major"):
            env.traj_layout = layout
            o, s, l = env.vmap_sim_ahead(to_state(env, st), torch.as_tensor(acts, device=env.device), env.tau, env.tau)
            o_ref, s_ref, l_ref = oracle.sim_ahead("pmsm", "euler", st, acts, props, spec["tau"], semantics=osem)
            ok = np.isfinite(o_ref).all(axis=(1, 2))
            assert ok.mean() > 0.9
            assert np.allclose(o.cpu().numpy()[ok], o_ref[ok], rtol=tol, atol=tol), (sem, layout)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("solver", ["euler", "tsit5"])
@pytest.mark.parametrize("motor", ["BRUSA", "SEW"])
def test_reference_motor_tables_step_and_sim_ahead_match_oracle(motor, solver, dtype):
    """The saturated model on the reference's OWN tables (tests/golden/pmsm/LUT_*_jax_grad.mat, loaded by the environment
    itself like pmsm_env.py:164-175 does): HIP kernels vs the CPU oracle, one step and both trajectory semantics. SEW brings its
    real NaN region (142 / 188 cells filled from the nearest node) and an i_d grid that reaches +1 A."""
    import os

    import exciting_environments_amd as ex
    from conftest import GOLDEN
    from exciting_environments_amd import EnvironmentRegistry, MotorVariant

    B, K = 2048, (40 if dtype == torch.float64 else 10)
    solv = {"euler": ex.Euler(), "rk4": ex.RK4(), "tsit5": ex.Tsit5()}[solver]
    env = EnvironmentRegistry.PMSM.make(batch_size=B, saturated=True, motor_variant=MotorVariant[motor], solver=solv, dtype=dtype,
                                        device="cuda", pmsm_lut_path=os.path.join(GOLDEN, "pmsm"))
    ep = env.env_properties
    params = {n: getattr(ep.static_params, n) for n in env.PARAM_FIELDS}
    pn = {n: (getattr(ep.physical_normalizations, n).min, getattr(ep.physical_normalizations, n).max) for n in env.STATE_FIELDS}
    an = {n: (getattr(ep.action_normalizations, n).min, getattr(ep.action_normalizations, n).max) for n in env.ACTION_FIELDS}
    props, keep = oracle.make_props("pmsm", params, pn, an, NP_DTYPE[dtype], B, pmsm_lut=env._lut_host)
    props64, keep64 = oracle.make_props("pmsm", params, pn, an, np.float64, B, pmsm_lut=env._lut_host)
    spec = dict(params=params, phys_norm=pn, act_norm=an, tau=env.tau)
    st = random_state("pmsm", B, NP_DTYPE[dtype], spec, seed=431)
    st[6] = (st[6] * (0.25 if motor == "BRUSA" else 0.1)).astype(NP_DTYPE[dtype])  # moderate speeds: the horizon stays bounded
    st[3][::7] = NP_DTYPE[dtype](pn["i_d"][0] * 1.6)   # beyond the table (constant extrapolation through the padded edge)
    st[4][3::11] = NP_DTYPE[dtype](pn["i_q"][1] * 1.3)
    rng = np.random.default_rng(432)
    acts = rng.uniform(-1, 1, (B, K, 2)).astype(NP_DTYPE[dtype])
    tol = 1e-9 if dtype == torch.float64 else 5e-5
    obs, new = env.vmap_step(to_state(env, st), torch.as_tensor(acts[:, 0], device=env.device))
    o_ref, s_ref = oracle.step("pmsm", solver, st, acts[:, 0], props, spec["tau"])
    assert np.isfinite(o_ref).all()
    assert np.allclose(obs.cpu().numpy(), o_ref, rtol=tol, atol=tol), float(np.abs(obs.cpu().numpy() - o_ref).max())
    assert np.allclose(new.physical_state.torque.cpu().numpy(), s_ref[5], rtol=tol, atol=tol * pn["torque"][1])
    # ---- (A) the arithmetic itself, free of amplification: ONE step from states along the oracle's own trajectory ----------
    # Where kernel and oracle separate was isolated in round 4 (tools/f3_divergence.py): one step from identical
    # states gives bit-identical epsilon, i_d, i_q, torque in every environment, both motors, Euler and Tsit5 — cell search,
    # bilinear blend, closed-form 2x2 inverse, invariant divisions and RK stage sums are the oracle's operations in the oracle's
    # order. The ONLY difference is the clipped voltage that goes into the dead-time buffer: sin / cos of the Park rotation come
    # from the device routines instead of libm (absolute <= 1e-15 of full scale in fp64). Everything a trajectory shows later is
    # that last-place difference amplified by the machine (x 4 ... x 10^4 per step at these operating points, measured on the
    # oracle itself), so the trajectory-level assertions below can only be loose; THIS one is exact.
    eps_w = np.finfo(NP_DTYPE[dtype]).eps
    o_tr, s_tr, _ = oracle.sim_ahead("pmsm", solver, st, acts, props, spec["tau"], semantics=oracle.SEM_STEP)
    exact_leaves = ("epsilon", "i_d", "i_q", "torque", "omega_el")
    rows = sorted(set(range(0, K, max(1, K // 8))) | {K - 1})
    for r in rows:
        st_r = [np.ascontiguousarray(x[:, r]) for x in s_tr]
        fin = np.all([np.isfinite(x) for x in st_r], axis=0) & np.all([np.isfinite(x[:, r + 1]) for x in s_tr], axis=0)
        assert fin.mean() > 0.9
        env.sim_ahead_semantics = "step"
        _, new = env.vmap_step(to_state(env, st_r), torch.as_tensor(acts[:, r], device=env.device))
        for j, n in enumerate(env.STATE_FIELDS):
            got, want = getattr(new.physical_state, n).cpu().numpy()[fin], s_tr[j][fin, r + 1]
            if n in exact_leaves:
                assert np.array_equal(got, want), (r, n, float(np.abs(got - want).max()))
            else:  # u_d_buffer / u_q_buffer: device sin / cos in the rotation of the clipped voltage
                assert np.abs(got - want).max() <= 16 * eps_w * pn[n][1], (r, n, float(np.abs(got - want).max()))
        # the reference-structured launch, one action row from the same states (row 1 is post-processed: wrapped angle, torque)
        env.sim_ahead_semantics = "ahead"
        o1, s1, _l1 = env.vmap_sim_ahead(to_state(env, st_r), torch.as_tensor(acts[:, r:r + 1], device=env.device), env.tau, env.tau)
        _o, s1_ref, _ = oracle.sim_ahead("pmsm", solver, st_r, acts[:, r:r + 1], props, spec["tau"], semantics=oracle.SEM_AHEAD)
        for j, n in enumerate(env.STATE_FIELDS):
            got, want = getattr(s1.physical_state, n).cpu().numpy()[fin, 1], s1_ref[j][fin, 1]
            if n in exact_leaves:
                assert np.array_equal(got, want), ("ahead", r, n, float(np.abs(got - want).max()))
            else:
                assert np.abs(got - want).max() <= 16 * eps_w * pn[n][1], ("ahead", r, n)
    # ---- (B) whole trajectories ------------------------------------------------------------------------------------------
    for sem, osem in (("step", oracle.SEM_STEP), ("ahead", oracle.SEM_AHEAD)):
        env.sim_ahead_semantics = sem
        a_dev = env.new_actions_buffer(K)
        a_dev.copy_(torch.as_tensor(acts, device=env.device))
        o, s, l = env.vmap_sim_ahead(to_state(env, st), a_dev, env.tau, env.tau)
        o_ref, s_ref, l_ref = oracle.sim_ahead("pmsm", solver, st, acts, props, spec["tau"], semantics=osem)
        assert np.isfinite(o_ref).all()
        err = np.abs(o.cpu().numpy() - o_ref)
        if dtype == torch.float64:
            # fixed bound on the horizon where it still means something: three saved rows (measured <= 6e-11, SEW Tsit5; the
            # oracle against itself from inputs one ulp away is at 5.5e-11 there and at 1e-6 by row 9)
            assert err[:, :4].max() <= 1e-9, (sem, err[:, :4].max(axis=(0, 2)).tolist())
            # beyond it: not worse than the machine's own amplification of a one-ulp change of the inputs
            o_pert = oracle.sim_ahead("pmsm", solver, [np.nextafter(x, np.inf) for x in st], acts, props, spec["tau"], semantics=osem)[0]
            nat = np.abs(o_pert - o_ref).max(axis=(0, 2))
            got = err.max(axis=(0, 2))
            assert np.all(got <= 16 * nat + 1e-9), (sem, got.tolist(), nat.tolist())
        else:
            # fp32: no fixed bound means anything here — one Tsit5 step of the SEW machine turns a last-place difference of the
            # clipped voltage (6e-8) into 1e-2 of full scale (its c = 1 stage already sees the voltage clipped in this very
            # step). Rows are held against the distance between the oracle's own fp32 and fp64 runs; the arithmetic is pinned
            # exactly by (A).
            o64 = oracle.sim_ahead("pmsm", solver, [x.astype(np.float64) for x in st], acts.astype(np.float64), props64,
                                   spec["tau"], semantics=osem)[0]
            nat = np.abs(o_ref.astype(np.float64) - o64).max(axis=(0, 2))            # per row: fp32 oracle vs fp64 oracle
            got = np.abs(o.cpu().numpy().astype(np.float64) - o64).max(axis=(0, 2))  # per row: fp32 kernel vs fp64 oracle
            assert np.all(got <= 4 * nat + tol), (sem, got.tolist(), nat.tolist())
        assert torch.equal(l.physical_state.i_d, s.physical_state.i_d[:, -1])
