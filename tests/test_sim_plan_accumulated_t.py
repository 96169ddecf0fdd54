"""The planner (csrc/sim_plan.hpp) for EXCENV_SEM_AHEAD_ACCUMULATED_T, checked without a GPU through the driver of
tests/test_sim_plan.py: exactly what EXCENV_SEM_AHEAD gets, except that the forms which assume one action row per step (row-major
action windows, fused env-major kernels) and the lean gym outputs are never chosen, and the launch name says which clock ran. Under
all three semantics, every plan of a wider sweep is one launch.hpp instantiates (sim_instantiated)."""
import subprocess

import pytest

from test_sim_plan import CASES, CXX, CSRC, DRIVER, EM_L, F32, F64, FIELDS, LANE, MODELS, TILED, facts

SEM_STEP, SEM_AHEAD, SEM_ACC_T = 0, 1, 2
GENERAL, LEAN, LEAN_GYM, AEM, EM, EM_GENERAL, EMR = range(7)
SUFFIX = "accumulated t)"

# the shapes of the existing table plus a sweep over models, dtypes, solvers, batch sizes, layouts, workspace and gym outputs
SHAPES = [f for _, f, _ in CASES]
for model in ("pendulum", "mass_spring_damper", "cartpole", "acrobot", "fluid_tank", "pmsm"):
    for dtype in (F32, F64):
        for solver in ("euler", "rk4", "tsit5"):
            for B in (2048, 1 << 18, 1 << 22):
                for al, tl in ((LANE, LANE), (EM_L, LANE), (EM_L, EM_L), (LANE, EM_L), (TILED, TILED)):
                    for gym in (0, 1):
                        for ws in (0, 1):
                            SHAPES.append(facts(model, dtype, solver, B=B, K=64, action_layout=al, traj_layout=tl, gym=gym,
                                                workspace=ws, workspace_bytes=(1 << 40) if ws else 0))
            SHAPES.append(facts(model, dtype, B=4096, K=64, per_env_props=1))
            SHAPES.append(facts(model, dtype, B=4096, K=64, n_control=1))
            SHAPES.append(facts(model, dtype, B=1 << 20, K=100, envs_per_lane=1))
# sim_instantiated's sweep: the shapes above plus the facts that pick the look-up model, the general kernel, the control-column fill
# and the lane width
SWEEP = list(SHAPES)
for model in MODELS:
    for lut in ((0, 1) if model == "pmsm" else (0,)):
        for dtype in (F32, F64):
            for solver in ("euler", "rk4", "tsit5"):
                for B in (2048, 1 << 22):
                    for al, tl in ((LANE, LANE), (EM_L, LANE), (EM_L, EM_L), (TILED, TILED)):
                        for gym in (0, 1):
                            for pe in (0, 1):
                                for nc in (0, 1):
                                    for epl in (0, 1, 2, 4):
                                        for ws in (0, 1):
                                            SWEEP.append(facts(model, dtype, solver, B=B, K=64, action_layout=al, traj_layout=tl, gym=gym,
                                                               lut=lut, per_env_props=pe, n_control=nc, envs_per_lane=epl, workspace=ws,
                                                               workspace_bytes=(1 << 40) if ws else 0))


def run_driver(tmp_path_factory, rows):
    d = tmp_path_factory.mktemp("sim_plan_acc_t")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    return out


def parse(line):
    nums, name = line.split("|")
    form, ws, V, threads, row_sync, _lds, split, _period, inst = map(int, nums.split())
    return dict(form=form, ws=ws, V=V, threads=threads, row_sync=row_sync, split=split, inst=inst, name=name)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    rows = []
    for f in SHAPES:
        for sem in (SEM_AHEAD, SEM_ACC_T):
            rows.append(" ".join(str(dict(f, semantics=sem)[n]) for n in FIELDS))
    out = run_driver(tmp_path_factory, rows)
    return [(f, parse(out[2 * i]), parse(out[2 * i + 1])) for i, f in enumerate(SHAPES)]


def test_every_plan_is_instantiated(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    sems = (SEM_STEP, SEM_AHEAD, SEM_ACC_T)
    rows = [" ".join(str(dict(f, semantics=sem)[n]) for n in FIELDS) for f in SWEEP for sem in sems]
    out = run_driver(tmp_path_factory, rows)
    missing = [(SWEEP[i // len(sems)], sems[i % len(sems)], line) for i, line in enumerate(out) if not parse(line)["inst"]]
    assert not missing, missing[:5]
    # the sweep reaches every form, the look-up model's and the 1024-thread ones included
    forms = {(parse(line)["form"], parse(line)["threads"]) for line in out}
    assert {(GENERAL, 256), (LEAN, 256), (LEAN, 1024), (LEAN_GYM, 256), (LEAN_GYM, 1024), (AEM, 256), (EM, 64), (EM_GENERAL, 64),
            (EMR, 64)} <= forms


def test_never_a_form_without_an_accumulated_time_instantiation(plans):
    forms = {acc["form"] for _, _, acc in plans}
    assert forms <= {GENERAL, LEAN}, forms
    assert forms == {GENERAL, LEAN}
    # ... while the same shapes do reach those forms under SEM_AHEAD
    assert {AEM, LEAN_GYM, EM, EMR} <= {ahead["form"] for _, ahead, _ in plans}


def test_gym_requests_take_the_general_kernel(plans):
    gym = [acc for f, _, acc in plans if f["gym"]]
    assert gym and all(acc["form"] == GENERAL and acc["V"] == 1 for acc in gym)


def test_same_plan_as_sem_ahead_where_that_is_general_or_lean(plans):
    same = 0
    for f, ahead, acc in plans:
        if ahead["form"] in (GENERAL, LEAN):
            assert (acc["form"], acc["ws"], acc["V"], acc["threads"], acc["row_sync"], acc["split"]) == \
                (ahead["form"], ahead["ws"], ahead["V"], ahead["threads"], ahead["row_sync"], ahead["split"]), f
            same += 1
    assert same > 100


def test_row_major_actions_go_through_the_workspace(plans):
    rm = [(f, a, acc) for f, a, acc in plans if f["action_layout"] == EM_L and f["traj_layout"] == LANE and f["workspace"]
          and not f["gym"]]
    assert any(a["form"] == AEM for _, a, _ in rm)
    assert all(acc["ws"] == 1 and acc["form"] == LEAN for _, _, acc in rm)


def test_names(plans):
    for f, ahead, acc in plans:
        assert acc["name"].endswith(SUFFIX), acc["name"]
        assert not ahead["name"].endswith(SUFFIX)
        if ahead["form"] in (GENERAL, LEAN):
            assert acc["name"] == ahead["name"][:-1] + ", " + SUFFIX or (ahead["ws"] and acc["name"] ==
                                                                          "transposition workspace + sim_ahead_kernel (accumulated t)")
    names = {acc["name"] for _, _, acc in plans}
    assert {"sim_ahead_kernel (V=4, accumulated t)", "sim_ahead_kernel (V=1, accumulated t)", "sim_ahead_kernel (general, accumulated t)",
            "sim_ahead_kernel (V=4, 1024 threads, accumulated t)", "transposition workspace + sim_ahead_kernel (accumulated t)"} <= names


def test_sem_ahead_names_unchanged(plans):
    """The plain SEM_AHEAD names are the ones tests/test_sim_plan.py pins (byte-identical strings)."""
    pinned = {c[2][-1] for c in CASES}
    assert {ahead["name"] for _, ahead, _ in plans} <= pinned | {"sim_ahead_kernel (V=2, 1024 threads)"}
