// Linearisation of excenv_step: what one excenv_step_jacobian call launches. Host-only and free of HIP, like step_vjp.hpp: the call
// record, the name of the form and the algorithmic bytes of step_jac_kernel (kernels_step_jac.hpp).
#pragma once
#include "sim_plan.hpp"

namespace excenv {

// The validated call (excenv_api.hip): `rows` steps of B environments each. Step n leads from state_in[j] + n * state_row_stride to
// state_out[j] + n * state_row_stride ([B] each) under the action row n / substeps.
struct StepJacCall {
  int solver, dtype;
  int64_t B, rows;
  int32_t substeps;
  const excenv_props_t* props;
  double dt, env_tau;                   // the solver's step and the environment's tau (PMSM's dead-time advance)
  const void* const* state_in;          // S pointers: the steps' starting states
  const void* const* state_out;         // S pointers: the states the forward returned
  int64_t state_row_stride;             // elements between two steps of a state leaf
  const void* action;                   // element (row k, component q, environment i) at k * a_row + q * a_comp + i * a_env
  int64_t a_row, a_comp, a_env;
  int row_kind;                         // EXCENV_JAC_STATE or EXCENV_JAC_OBS
  void* jacobian;                       // [rows][R][S + A][B]
  int V;                                // step instances per lane: 1 (the only form built)
  void* stream;                         // hipStream_t
};

// step_jac_kernel<M, T, SOLVER> exists for every model but the saturated PMSM, the three solvers and both element types, one step
// instance per lane. `forced` is excenv_launch_opts_t.envs_per_lane (0: auto). Returns 0 when a forced width cannot be had.
constexpr int step_jac_envs_per_lane(int forced) { return (forced == 0 || forced == 1) ? 1 : 0; }

constexpr const char* step_jac_name(int row_kind) {
  return row_kind == EXCENV_JAC_OBS ? "step_jac_kernel (V=1, observation rows)" : "step_jac_kernel (V=1, state rows)";
}

// Jacobian rows of a step instance: one per state leaf or one per observation column of the model (reference columns have none)
constexpr int step_jac_rows(int S, int O, int row_kind) { return row_kind == EXCENV_JAC_OBS ? O : S; }

// Algorithmic bytes per step instance: both saved states and the action in, R rows of S + A entries out
constexpr int64_t step_jac_bytes(int S, int A, int O, int elem, int row_kind) {
  return (int64_t)elem * (2 * S + A + (int64_t)step_jac_rows(S, O, row_kind) * (S + A));
}

}  // namespace excenv
