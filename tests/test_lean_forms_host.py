"""The host half of the lean forward sweep (tests/helpers_forms.py, tests/test_gpu_lean_forms.py), without a GPU.

Completeness: sim_plan.hpp is compiled with the host C++ compiler (like tests/test_sim_plan.py) and sim_instantiated() is enumerated
over every environment id, element size, solver, semantics, lane width and look-up flag for the 256-thread LEAN form. That set must
equal the set of instantiations the sweep's case list launches, minus what the API refuses by name (helpers_forms.REFUSED): a new
lean instantiation fails here until the sweep covers it.

Finiteness: the oracle alone on every input of the sweep for the linear models: every observation and state it returns is finite, so
a comparison with it on the GPU compares numbers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from helpers_forms import (B, B_STEP_DOWN, LINEAR_CASES, LUT_LDS_LIMIT, MODEL_CASES, REFUSED, SEM_ID, SEMANTICS, cases, case_id, inputs,
                           instantiation_keys, linear_spec, lut_bytes, refused_key, saturated_tables, shapes, sim_forms, step_forms)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exciting-environments_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")

# every (env, elem, solver, semantics, V, lut) whose 256-thread LEAN plan launch.hpp instantiates, one per line; then the block size
ENUMERATE = r"""
#include <cstdio>
#include <initializer_list>
#include "sim_plan.hpp"
int main() {
  using namespace excenv;
  const int A[EXCENV_NUM_ENVS] = {1, 1, 1, 1, 1, 2};
  for (int env = 0; env < EXCENV_NUM_ENVS; ++env)
    for (int elem : {4, 8})
      for (int solver = 0; solver < EXCENV_NUM_SOLVERS; ++solver)
        for (int sem = EXCENV_SEM_STEP; sem <= EXCENV_SEM_AHEAD_ACCUMULATED_T; ++sem)
          for (int V : {1, 2, 4})
            for (int lut = 0; lut < 2; ++lut)
              if (sim_instantiated(SimPlan{SIM_LEAN, false, V, BLOCK, 0, 0, false, 0, sem == EXCENV_SEM_AHEAD_ACCUMULATED_T}, sem, env,
                                   A[env], elem, solver, lut != 0))
                std::printf("%d %d %d %d %d %d\n", env, elem, solver, sem, V, lut);
  std::printf("block %d\n", BLOCK);
}
"""


@pytest.fixture(scope="module")
def instantiated(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("lean_forms")
    src, exe = d / "enumerate.cpp", d / "enumerate"
    src.write_text(ENUMERATE)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1].split()[0] == "block"
    return {tuple(map(int, l.split())) for l in lines[:-1]}, int(lines[-1].split()[1])


def test_the_sweep_launches_every_lean_instantiation(instantiated):
    keys, block = instantiated
    assert oracle.ENV_IDS == {"pendulum": 0, "mass_spring_damper": 1, "cartpole": 2, "acrobot": 3, "fluid_tank": 4, "pmsm": 5}
    refused = {k for k in keys if refused_key(k[0], k[5])}
    swept = instantiation_keys()
    assert swept == keys - refused, (sorted(keys - refused - swept), sorted(swept - (keys - refused)))
    # 7 models (PMSM with and without tables) x 3 solvers x 3 semantics x (V = 1, 2, 4 in fp32 + V = 1, 2 in fp64)
    assert len(swept) == 7 * 3 * 3 * 5 == 315
    # each of them with and without state trajectories; the look-up model's once more per place its tables live in
    launched = sum(len(sim_forms(d)) for _, _, d in cases())
    assert launched == 9 * 3 * 3 * 5 * 2 == 810
    assert sum(len(step_forms(d)) for _, _, d in cases()) == 9 * 3 * 5 == 135
    assert all(len(r) == 2 and r[1] for r in REFUSED)
    # the batch is what the sweep's docstrings say it is for this block size
    assert block == 256 and B == 4 * 326 and B % 64 != 0
    assert (B // 4 + block - 1) // block == 2 and (B // 4) % 64 == 6  # one full workgroup ... and six lanes of a wave of the next
    assert (B // 2 + block - 1) // block == 3 and (B // 2) % block != 0
    assert (B + block - 1) // block == 6 and B % block == 24
    assert B_STEP_DOWN % 4 != 0 and B_STEP_DOWN % 2 == 0


@pytest.mark.parametrize("model_case", [m for m in MODEL_CASES if m not in LINEAR_CASES])
def test_the_saturated_tables_live_where_the_case_says(model_case):
    from exciting_environments_amd import prepare_pmsm_lut

    prepared = prepare_pmsm_lut(saturated_tables(model_case))
    for elem in (4, 8):
        fits = lut_bytes(prepared, elem) <= LUT_LDS_LIMIT
        assert fits == (MODEL_CASES[model_case][2] == "lds"), (model_case, elem, lut_bytes(prepared, elem))


@pytest.mark.parametrize("case", [c for c in cases() if c[0] in LINEAR_CASES], ids=case_id)
def test_the_oracle_is_finite_on_every_input_of_the_sweep(case):
    model_case, solver, dtype = case
    env_name = MODEL_CASES[model_case][0]
    spec = linear_spec(model_case)
    for batch in (B, B_STEP_DOWN):
        st, acts = inputs(model_case, spec, dtype, batch)
        props, keep = oracle.make_props(env_name, spec["params"], spec["phys_norm"], spec["act_norm"], np.dtype(dtype), batch)
        obs, new = oracle.step(env_name, solver, st, acts[:, 0], props, spec["tau"])
        assert np.isfinite(obs).all() and all(np.isfinite(x).all() for x in new)
        for sem in SEMANTICS:
            for K, sub in shapes(model_case):
                o, s, l = oracle.sim_ahead(env_name, solver, st, acts[:, :K], props, spec["tau"] / sub, env_tau=spec["tau"], substeps=sub,
                                           semantics=SEM_ID[sem])
                assert o.shape[:2] == (batch, K * sub + 1)
                assert np.isfinite(o).all() and all(np.isfinite(x).all() for x in s) and all(np.isfinite(x).all() for x in l), (sem, K, sub)
