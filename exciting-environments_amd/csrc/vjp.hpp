// Reverse mode of excenv_sim_ahead: what one excenv_sim_ahead_vjp call launches. Host-only and free of HIP, like sim_plan.hpp: the
// call record, the form (environments per lane) and which instantiations of sim_ahead_vjp_kernel (kernels_vjp.hpp) exist.
#pragma once
#include "sim_plan.hpp"

namespace excenv {

// The validated call (excenv_api.hip): everything lane-major, actions already in [K][A][B] order
struct VjpCall {
  int solver, dtype;
  int64_t B, K;
  int32_t substeps, n_control;
  const excenv_props_t* props;
  double obs_stepsize, env_tau;
  int semantics;                        // EXCENV_SEM_STEP or EXCENV_SEM_AHEAD
  const void* actions;                  // [K][A][B]
  const void* const* state_traj;        // S x [N + 1][B]: the rows the forward call saved
  const void* grad_obs_traj;            // [N + 1][O + n_control][B] or nullptr
  const void* const* grad_state_traj;   // nullptr, or S pointers ([N + 1][B] or nullptr each)
  const void* const* grad_last_state;   // nullptr, or S pointers ([B] or nullptr each)
  void* grad_actions;                   // [K][A][B]
  void* const* grad_state_in;           // S x [B]
  int V;                                // environments per lane (vjp_envs_per_lane)
  void* raw_rows;                       // [N + 1][B] workspace where vjp_needs_raw_rows, else nullptr
  void* stream;                         // hipStream_t
  void* const* grad_params = nullptr;   // excenv_sim_ahead_vjp_params: EXCENV_MAX_STATIC pointers ([B] or nullptr each); else nullptr
};

// The wide form (16 bytes per lane) keeps 16 / elem environments' rows, cotangents and accumulators in registers next to one
// environment's stages: it exists where that fits the register file without scratch (tools/loop_code_size.py kernel_resources) —
// every solver of the three small models, the Euler kernels of cart-pole, and of acrobot and PMSM with 4-byte elements.
constexpr bool vjp_wide_ok(int env, int elem, int solver) {
  if (env == EXCENV_PENDULUM || env == EXCENV_MASS_SPRING_DAMPER || env == EXCENV_FLUID_TANK) return true;
  if (solver != EXCENV_EULER) return false;
  return env == EXCENV_CART_POLE || elem == 4;
}
// The PGRAD instantiations (gradients w.r.t. the static parameters) carry P x V more accumulators through the trajectory: their
// wide form exists where the built library still meets the budget above with them (DESIGN.md §4.9 "Parameter gradients"); a call
// whose model has no wide PGRAD form runs one environment per lane.
constexpr bool vjp_pgrad_wide_ok(int env, int elem, int solver) {
  return vjp_wide_ok(env, elem, solver) && env != EXCENV_PMSM;  // PMSM Euler fp32: 229 / 235 registers + 5 x 4 accumulators spill
}
// sim_ahead_vjp_kernel<M, T, SOLVER, AHEAD, V, PGRAD> exists for every model but the saturated PMSM, the three solvers, both
// semantics with a fixed step, one environment per lane and (vjp_wide_ok / vjp_pgrad_wide_ok) 16 bytes per lane
constexpr bool vjp_instantiated(int semantics, int env, int elem, int solver, bool lut, int V, bool pgrad = false) {
  if (lut || (elem != 4 && elem != 8) || solver < 0 || solver >= EXCENV_NUM_SOLVERS) return false;
  if (semantics != EXCENV_SEM_STEP && semantics != EXCENV_SEM_AHEAD) return false;
  return V == 1 || (V == 16 / elem && (pgrad ? vjp_pgrad_wide_ok(env, elem, solver) : vjp_wide_ok(env, elem, solver)));
}
// Which static-parameter leaves have a gradient: every floating leaf of the six models; PMSM's p and deadtime are integers
constexpr bool vjp_param_differentiable(int env, int index) { return !(env == EXCENV_PMSM && (index == 0 || index == 6)); }

// Environments per lane: the forward's own batch rule (auto_envs_per_lane) decides between the two forms; `forced` is
// excenv_launch_opts_t.envs_per_lane (0: auto). `wide_ok`: B % (16 / elem) == 0 and every array 16-byte aligned (and the model has the form).
// Returns 0 when a forced width cannot be had.
constexpr int vjp_envs_per_lane(int env, int solver, int64_t B, int elem, int forced, bool wide_ok, bool pgrad = false) {
  const int vmax = 16 / elem;
  wide_ok = wide_ok && (pgrad ? vjp_pgrad_wide_ok(env, elem, solver) : vjp_wide_ok(env, elem, solver));
  if (forced == 1) return 1;
  if (forced > 0) return (forced == vmax && wide_ok) ? vmax : 0;
  return (wide_ok && auto_envs_per_lane(B, vmax) == vmax) ? vmax : 1;
}

// Workspace of a call whose actions are row-major [B][K][A]: their lane-major copy
constexpr int64_t vjp_workspace_bytes(int A, int elem, int64_t B, int64_t K, int action_layout) {
  return action_layout == EXCENV_LAYOUT_ENV_MAJOR ? align_up(elem * K * A * B) : 0;
}

// The saved rows are the reverse pass's checkpoints, and under EXCENV_SEM_AHEAD they are post-processed copies of the raw state the
// forward carries. For the tank that copy loses what an RK step starts from: a level that ran below 0 is saved as 0, and a stage
// state built from 0 is not the one built from the raw level (it may be wet where the raw one is dry). Those calls re-simulate the
// raw levels first (vjp_raw_rows_kernel) into a second part of the workspace, behind the transposed actions. Euler's only stage
// state is the row itself, which f reads as max(h, 0): nothing to restore. No other model's post-processing changes a Jacobian.
constexpr bool vjp_needs_raw_rows(int env, int solver, int semantics) {
  return env == EXCENV_FLUID_TANK && solver != EXCENV_EULER && semantics == EXCENV_SEM_AHEAD;
}
constexpr int64_t vjp_raw_rows_bytes(int env, int solver, int semantics, int elem, int64_t B, int64_t K, int32_t substeps) {
  return vjp_needs_raw_rows(env, solver, semantics) ? align_up(elem * (K * substeps + 1) * B) : 0;
}

constexpr const char* vjp_name(int V, bool pgrad = false) {
  if (pgrad) return V == 1 ? "sim_ahead_vjp_kernel (V=1, PGRAD)" : V == 2 ? "sim_ahead_vjp_kernel (V=2, PGRAD)" : "sim_ahead_vjp_kernel (V=4, PGRAD)";
  return V == 1 ? "sim_ahead_vjp_kernel (V=1)" : V == 2 ? "sim_ahead_vjp_kernel (V=2)" : "sim_ahead_vjp_kernel (V=4)";
}

// ---- the deterministic batch sum of per-environment gradients (param_sum.hip) ------------------------------------------------
// Stage one: PSUM_GROUPS workgroups of PSUM_BLOCK lanes (fewer for a small batch: one workgroup per PSUM_SLICE environments),
// each over a fixed slice of [B], one fp64 partial per workgroup and leaf. Stage two: one workgroup adds the partials in order.
constexpr int PSUM_BLOCK = 256, PSUM_GROUPS = 256, PSUM_SLICE = 4096;
constexpr int param_sum_groups(int64_t B) {
  const int64_t g = (B + PSUM_SLICE - 1) / PSUM_SLICE;
  return g < 1 ? 1 : g > PSUM_GROUPS ? PSUM_GROUPS : (int)g;
}
constexpr int64_t param_sum_workspace_bytes(int64_t B, int n) { return align_up((int64_t)8 * param_sum_groups(B) * (n > 0 ? n : 1)); }

}  // namespace excenv
