"""Every lean (vectorised, GENERAL = false) instantiation of sim_ahead_kernel and step_kernel, form by form (``-m gpu``).

The case list is tests/helpers_forms.py (tests/test_lean_forms_host.py proves it complete against sim_instantiated()): nine model
cases — the five small models, PMSM with dead time 1 and 0, the saturated PMSM with its tables in LDS and in global memory — x three
solvers x two dtypes. Models are off their defaults with asymmetric ranges (helpers_vjp.skewed_spec); normalised actions reach
+-1.1. Per case every form is launched on the same inputs: the three semantics x 1 / 2 / 4 (fp32) environments per lane x state
trajectories on / off at K = 1, 2, 9 (no next action row, exactly one, both parities of the ping-pong action registers) and, where the
model has substeps, K = 3 x 3; vmap_step at every lane width. B = 1304 = 4 * 326 for every width: one workgroup, one wave and six
lanes at four per lane; two workgroups and a ragged tail at two; five workgroups and 24 lanes at one. At B = 1302 a request for the
widest lane must run two per lane.

Per launch:
(a) excenv_last_launch() names the form that was asked for — a silent fallback to a narrower one fails;
(b) observations, state trajectory (where written) and last state of every launch are torch.equal to the one-per-lane, states-on
    launch of the same semantics and shape (the lane widths are bit-identical), without tolerance;
(c) that one-per-lane launch of the linear models is held against the CPU oracle on the same skewed specification with the bounds of
    tests/test_gpu_parity.py (imported: identical bits for mass-spring-damper and tank, 1e-9 in fp64, 1e-5 in fp32, angles on the
    circle). The saturated model gets (a) and (b): its one-per-lane kernel is pinned by tests/test_gpu_saturated.py, which explains
    why no fixed trajectory bound means anything for that machine in fp32.

Every case prints the names it asserted and its largest distance from the oracle (next to the distance between the oracle's own fp32
and fp64 runs on the same inputs under "step" / "ahead", the reference's own error). Measured on an MI355X: every
form has the bits of its one-per-lane launch; trajectories fp64 <= 1.6e-15, fp32 <= 9.5e-7 (PMSM Tsit5 both; the oracle's fp32 and
fp64 runs are 3.8e-7 ... 3.1e-6 apart), one step fp64 <= 6.7e-16, fp32 <= 3.0e-7 — the fp32 bound of 1e-5, measured before on
default models over 64 steps, holds on the skewed ones unchanged."""
import numpy as np
import pytest
import torch

import oracle
from helpers import ANGLE_OBS, ANGLE_STATES, circ_close, make_env, to_state
from helpers_forms import (B, B_STEP_DOWN, K_MAX, MODEL_CASES, SEM_ID, SEMANTICS, case_id, cases, inputs, lane_widths, linear_spec,
                           saturated_tables, shapes, sim_name, step_forms, step_name)
from helpers_lut import make_saturated
from test_gpu_parity import _close, _tol

pytestmark = pytest.mark.gpu


def _build(model_case, solver, dtype, batch):
    """-> env, oracle props (None for the saturated model: no oracle comparison), keepalive, spec, states, actions"""
    env_name, _, lut = MODEL_CASES[model_case]
    if lut is None:
        spec = linear_spec(model_case)
        env, props, keep, spec = make_env(env_name, batch, dtype, solver, spec=spec)
    else:
        env, _, keep, spec = make_saturated(batch, dtype, solver, saturated_tables(model_case))
        props = None
    st, acts = inputs(model_case, spec, str(dtype).split(".")[1], batch)
    return env, props, keep, spec, st, acts


def _obs_dist(env_name, got, want):
    """largest |difference| of normalised observations, wrapped angles on the circle"""
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    for c in ANGLE_OBS.get(env_name, []):
        d[..., c] = np.minimum(d[..., c], np.abs(2.0 - d[..., c]))
    return float(d.max())


def _states_close(env_name, got, want, dtype):
    """the state leaves against the oracle's as tests/test_gpu_parity.py holds them -> names of the leaves that miss the bound"""
    rtol, atol = _tol(env_name, dtype)
    bad = []
    for j, n in enumerate(oracle.STATE_FIELDS[env_name]):
        g, w = np.asarray(got[j]), np.asarray(want[j])
        scale = max(1.0, float(np.nanmax(np.abs(w))))
        if rtol == 0:
            ok = np.array_equal(g, w)
        elif j in ANGLE_STATES.get(env_name, []):
            ok = circ_close(g[..., None], w[..., None], [0], rtol, atol * scale, period=2 * np.pi)
        else:
            ok = np.allclose(g, w, rtol=rtol, atol=atol * scale)
        if not ok:
            bad.append(n)
    return bad


def _leaves(env, tree):
    return [getattr(tree.physical_state, n) for n in env.STATE_FIELDS]


def _oracle64(env_name, spec, batch):
    return oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.float64, batch)


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_sim_ahead_forms(case):
    from exciting_environments_amd import _native

    model_case, solver, dtype_name = case
    dtype = getattr(torch, dtype_name)
    env_name = MODEL_CASES[model_case][0]
    widths = lane_widths(dtype_name)
    problems, names, dist, ref_dist = [], set(), 0.0, 0.0
    # the whole form list at B; at B_STEP_DOWN the widest request alone (it must run two per lane), one shape
    for batch, asked, shape_list in ((B, widths, shapes(model_case)), (B_STEP_DOWN, [1, widths[-1]], [(K_MAX, 1)])):
        env, props, keep, spec, st, acts = _build(model_case, solver, dtype, batch)
        if props is not None and dtype is torch.float32:
            props64, keep64 = _oracle64(env_name, spec, batch)
        state = to_state(env, st)
        for K, sub in shape_list:
            a = env.new_actions_buffer(K)
            a.copy_(torch.as_tensor(acts[:, :K], device=env.device))
            for sem in SEMANTICS:
                env.sim_ahead_semantics = sem
                ref = None
                for V in asked:
                    runs = min(V, 2) if batch == B_STEP_DOWN else V
                    for states_on in (True, False):
                        where = f"B={batch} K={K} substeps={sub} {sem} V={V} states={'on' if states_on else 'off'}"
                        env.store_state_trajectory = states_on
                        env.launch_opts = _native.launch_opts(envs_per_lane=V)
                        obs, traj, last = env.vmap_sim_ahead(state, a, env.tau / sub, env.tau)
                        name = _native.last_launch()
                        names.add(name)
                        assert name == sim_name(runs, sem), (where, name)                                   # (a)
                        assert tuple(obs.shape[:2]) == (batch, K * sub + 1) and (traj is not None) == states_on, where
                        if ref is None:
                            ref = (obs, _leaves(env, traj), _leaves(env, last))
                            assert bool(torch.isfinite(obs).all()), where
                            continue
                        if not torch.equal(obs, ref[0]):                                                   # (b)
                            problems.append(f"{where}: observations differ from V=1 by {(obs - ref[0]).abs().max().item():.3e}")
                        if states_on and not all(torch.equal(x, y) for x, y in zip(_leaves(env, traj), ref[1])):
                            problems.append(f"{where}: state trajectory differs from V=1")
                        if not all(torch.equal(x, y) for x, y in zip(_leaves(env, last), ref[2])):
                            problems.append(f"{where}: last state differs from V=1")
                if props is None:
                    continue
                where = f"B={batch} K={K} substeps={sub} {sem} V=1"                                           # (c)
                o_ref, s_ref, l_ref = oracle.sim_ahead(env_name, solver, st, acts[:, :K], props, spec["tau"] / sub, env_tau=spec["tau"],
                                                       substeps=sub, semantics=SEM_ID[sem])
                got = ref[0].cpu().numpy()
                d = _obs_dist(env_name, got, o_ref)
                dist = max(dist, d)
                # (on the accumulated-time clock fp32 and fp64 read different action rows by design: no reference error to measure)
                if dtype is torch.float32 and sem != "ahead_accumulated_t":
                    o64 = oracle.sim_ahead(env_name, solver, [x.astype(np.float64) for x in st], acts[:, :K].astype(np.float64), props64,
                                           spec["tau"] / sub, env_tau=spec["tau"], substeps=sub, semantics=SEM_ID[sem])[0]
                    ref_dist = max(ref_dist, _obs_dist(env_name, o_ref, o64))
                if not _close(env_name, got, o_ref, dtype):
                    problems.append(f"{where}: observations miss the oracle bound, distance {d:.3e}")
                bad = _states_close(env_name, [x.cpu().numpy() for x in ref[1]], s_ref, dtype)
                bad += [n + " (last)" for n in _states_close(env_name, [x.cpu().numpy() for x in ref[2]], l_ref, dtype)]
                if bad:
                    problems.append(f"{where}: state leaves {bad} miss the oracle bound")
    print(f"lean forms {case_id(case)}: asserted {sorted(names)}; "
          + ("no oracle comparison (saturated model)" if props is None else
             f"largest distance from the oracle {dist:.3e}" + (f", fp32 oracle from fp64 oracle {ref_dist:.3e}" if dtype is torch.float32 else "")))
    assert not problems, problems


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_step_forms(case):
    from exciting_environments_amd import _native

    model_case, solver, dtype_name = case
    dtype = getattr(torch, dtype_name)
    env_name = MODEL_CASES[model_case][0]
    widths = step_forms(dtype_name)
    problems, names, dist, ref_dist = [], set(), 0.0, 0.0
    for batch, asked in ((B, widths), (B_STEP_DOWN, [1, widths[-1]])):
        env, props, keep, spec, st, acts = _build(model_case, solver, dtype, batch)
        state = to_state(env, st)
        act = torch.as_tensor(acts[:, 0].copy(), device=env.device)
        ref = None
        for V in asked:
            runs = min(V, 2) if batch == B_STEP_DOWN else V
            env.launch_opts = _native.launch_opts(envs_per_lane=V)
            obs, new = env.vmap_step(state, act)
            name = _native.last_launch()
            names.add(name)
            assert name == step_name(runs), (batch, V, name)                                                # (a)
            if ref is None:
                ref = (obs, _leaves(env, new))
                assert bool(torch.isfinite(obs).all()), (batch, V)
                continue
            if not torch.equal(obs, ref[0]):                                                               # (b)
                problems.append(f"B={batch} V={V}: observations differ from V=1 by {(obs - ref[0]).abs().max().item():.3e}")
            if not all(torch.equal(x, y) for x, y in zip(_leaves(env, new), ref[1])):
                problems.append(f"B={batch} V={V}: new state differs from V=1")
        if props is None:
            continue
        o_ref, s_ref = oracle.step(env_name, solver, st, acts[:, 0], props, spec["tau"])                     # (c)
        got = ref[0].cpu().numpy()
        d = _obs_dist(env_name, got, o_ref)
        dist = max(dist, d)
        if dtype is torch.float32:
            props64, keep64 = _oracle64(env_name, spec, batch)
            o64 = oracle.step(env_name, solver, [x.astype(np.float64) for x in st], acts[:, 0].astype(np.float64), props64, spec["tau"])[0]
            ref_dist = max(ref_dist, _obs_dist(env_name, o_ref, o64))
        if not _close(env_name, got, o_ref, dtype):
            problems.append(f"B={batch} V=1: observations miss the oracle bound, distance {d:.3e}")
        bad = _states_close(env_name, [x.cpu().numpy() for x in ref[1]], s_ref, dtype)
        if bad:
            problems.append(f"B={batch} V=1: state leaves {bad} miss the oracle bound")
    print(f"lean forms step {case_id(case)}: asserted {sorted(names)}; "
          + ("no oracle comparison (saturated model)" if props is None else
             f"largest distance from the oracle {dist:.3e}" + (f", fp32 oracle from fp64 oracle {ref_dist:.3e}" if dtype is torch.float32 else "")))
    assert not problems, problems
