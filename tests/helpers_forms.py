"""The case list of the lean forward sweep, shared by its host half (tests/test_lean_forms_host.py: completeness against
sim_instantiated(), the oracle finite on every input) and its GPU half (tests/test_gpu_lean_forms.py: every lean instantiation of
sim_ahead_kernel and step_kernel against the one-environment-per-lane form and the oracle).

A case is (model case, solver, dtype). Per case the sweep launches every FORM: for vmap_sim_ahead the three semantics x the lane
widths of the dtype x state trajectories on / off, for vmap_step the lane widths. Models are moved off their defaults
(helpers_vjp.skewed_spec); the saturated PMSM keeps the motor's own parameters (helpers_lut.make_saturated)."""
import numpy as np

import oracle
from helpers import random_state
from helpers_vjp import skewed_spec

# model case -> (environment, dead time | None, look-up tables: None | "lds" | "global")
MODEL_CASES = {
    "pendulum": ("pendulum", None, None),
    "mass_spring_damper": ("mass_spring_damper", None, None),
    "cartpole": ("cartpole", None, None),
    "acrobot": ("acrobot", None, None),
    "fluid_tank": ("fluid_tank", None, None),
    "pmsm_deadtime1": ("pmsm", 1, None),
    "pmsm_deadtime0": ("pmsm", 0, None),
    "pmsm_saturated_lds": ("pmsm", None, "lds"),        # helpers_lut.saturating_lut(): 26 x 51 tables, staged in LDS
    "pmsm_saturated_global": ("pmsm", None, "global"),  # 81 x 81 tables: larger than LDS in either dtype, read from global memory
}
LINEAR_CASES = [m for m, (_, _, lut) in MODEL_CASES.items() if lut is None]
SOLVERS = ["euler", "rk4", "tsit5"]
DTYPES = ["float32", "float64"]
SEMANTICS = ["step", "ahead", "ahead_accumulated_t"]
SEM_ID = {"step": oracle.SEM_STEP, "ahead": oracle.SEM_AHEAD, "ahead_accumulated_t": oracle.SEM_AHEAD_ACCUMULATED_T}
ELEM = {"float32": 4, "float64": 8}

# B = 4 * 326 for every lane width, so that all forms see the same inputs: four per lane one workgroup (one full wave, six lanes of
# a third), two per lane two workgroups and a ragged tail, one per lane five workgroups and 24 lanes
B = 1304
B_STEP_DOWN = 1302  # no multiple of four: a request for four per lane runs two (plan_lane_major steps the width down)
K_MAX = 9
ACTION_RANGE = 1.1  # normalised actions in [-1.1, 1.1]: the clip of the action is part of every step
LUT_LDS_LIMIT = 150 * 1024  # launch.hpp lut_lds_bytes: tables up to this size are staged in LDS

# What the API refuses by name, and so what no case can launch. Only the first removes instantiation keys from the sweep; the other
# two bound the model cases (dead time 0 and 1) and the shapes (PMSM without substeps).
REFUSED = [
    ("look-up tables with a model other than PMSM", "pmsm_lut is only valid for EXCENV_PMSM"),
    ("PMSM with dead time > 1 under 'ahead' / 'ahead_accumulated_t'", "PMSM: EXCENV_SEM_AHEAD supports deadtime 0 or 1"),
    ("PMSM with obs_stepsize < action_stepsize", "PMSM: obs_stepsize must equal action_stepsize"),
]


def cases():
    """(model case, solver, dtype): one pytest case of the sim_ahead sweep and one of the step sweep each"""
    return [(m, s, d) for m in MODEL_CASES for s in SOLVERS for d in DTYPES]


def case_id(case):
    return "-".join(case)


def lane_widths(dtype):
    """environments per lane: 16 bytes per lane at the most"""
    return [1, 2, 4] if dtype == "float32" else [1, 2]


def sim_forms(dtype):
    """(semantics, environments per lane, state trajectories written) of one case; the first of each semantics is the one-per-lane,
    states-on launch the others are compared with"""
    return [(sem, V, states) for sem in SEMANTICS for V in lane_widths(dtype) for states in (True, False)]


def step_forms(dtype):
    return lane_widths(dtype)


def shapes(model_case):
    """(K, substeps): no next action row, exactly one, both parities of the ping-pong action registers; substeps where the model
    has them"""
    out = [(1, 1), (2, 1), (9, 1)]
    if MODEL_CASES[model_case][0] != "pmsm":
        out.append((3, 3))
    return out


def instantiation_keys():
    """What the sweep launches, as sim_instantiated()'s arguments: (env id, element size, solver id, semantics id, V, look-up)"""
    keys = set()
    for m, solver, dtype in cases():
        env_name, _, lut = MODEL_CASES[m]
        for sem, V, _ in sim_forms(dtype):
            keys.add((oracle.ENV_IDS[env_name], ELEM[dtype], oracle.SOLVER_IDS[solver], SEM_ID[sem], V, int(lut is not None)))
    return keys


def refused_key(env_id, lut):
    """REFUSED[0] as a predicate on an instantiation key"""
    return bool(lut) and env_id != oracle.ENV_IDS["pmsm"]


def linear_spec(model_case):
    env_name, deadtime, lut = MODEL_CASES[model_case]
    assert lut is None
    return skewed_spec(env_name, deadtime)


def saturated_tables(model_case):
    from exciting_environments_amd import MotorVariant
    from helpers_lut import linear_lut, saturating_lut

    kind = MODEL_CASES[model_case][2]
    if kind == "lds":
        return saturating_lut()
    sp = MotorVariant.BRUSA.get_params().static_params
    return linear_lut(sp["l_d"], sp["l_q"], sp["psi_p"], i_d_range=(-2000, 2000), i_q_range=(-2000, 2000), n_d=81, n_q=81)


def lut_bytes(prepared, elem):
    """launch.hpp lut_lds_bytes: tables, grids and cell-width reciprocals of prepare_pmsm_lut()'s (grid_d, grid_q, tables)"""
    n_d, n_q = len(prepared[0]), len(prepared[1])
    return (n_d * n_q * 8 + 2 * (n_d + n_q)) * elem


def inputs(model_case, spec, dtype, batch=B):
    """Seeded states inside the (skewed) normalisation box and K_MAX action rows; a shape with fewer rows takes the first K"""
    env_name = MODEL_CASES[model_case][0]
    npdt = np.dtype(dtype).type
    seed = 1000 + 10 * list(MODEL_CASES).index(model_case)
    st = random_state(env_name, batch, npdt, spec, seed=seed)
    A = len(oracle.ACTION_FIELDS[env_name])
    acts = np.random.default_rng(seed + 1).uniform(-ACTION_RANGE, ACTION_RANGE, (batch, K_MAX, A)).astype(npdt)
    return st, acts


def sim_name(V, semantics):
    return f"sim_ahead_kernel (V={V}, accumulated t)" if semantics == "ahead_accumulated_t" else f"sim_ahead_kernel (V={V})"


def step_name(V):
    return f"step_kernel (V={V})"
