// Reverse mode of one excenv_step / excenv_gym_step: what one excenv_step_vjp call launches. Host-only and free of HIP, like vjp.hpp:
// the call record, the name of the form and the algorithmic bytes of step_vjp_kernel (kernels_step_vjp.hpp).
#pragma once
#include "sim_plan.hpp"

namespace excenv {

// The validated call (excenv_api.hip): [B] state leaves, row-major action and observation cotangent as excenv_step takes / writes them
struct StepVjpCall {
  int solver, dtype;
  int64_t B;
  const excenv_props_t* props;
  const excenv_control_t* control;      // nullptr when n_control == 0; the references are read only with a reward cotangent
  double tau;
  const void* const* state_in;          // S x [B]: the step's starting state
  const void* action;                   // [B][A]
  const void* const* state_out;         // S x [B]: the state the forward step returned
  const void* grad_obs;                 // [B][O + n_control] or nullptr
  const void* const* grad_state_out;    // nullptr, or S pointers ([B] or nullptr each)
  const void* grad_reward;              // [B] or nullptr
  void* const* grad_state_in;           // S x [B]
  void* grad_action;                    // [B][A]
  int V;                                // environments per lane: 1 (the only form built)
  void* stream;                         // hipStream_t
};

// step_vjp_kernel<M, T, SOLVER, V> exists for every model but the saturated PMSM, the three solvers, both element types and one
// environment per lane. `forced` is excenv_launch_opts_t.envs_per_lane (0: auto). Returns 0 when a forced width cannot be had.
constexpr int step_vjp_envs_per_lane(int forced) { return (forced == 0 || forced == 1) ? 1 : 0; }

constexpr const char* step_vjp_name(int V) { return V == 1 ? "step_vjp_kernel (V=1)" : "step_vjp_kernel (?)"; }

// Algorithmic bytes per environment (DESIGN.md §4.9 "Step"): both saved states and the action in, the cotangent groups that are
// present (the reward's brings the references of the controlled fields), the two gradients out
constexpr int64_t step_vjp_bytes(int S, int A, int O, int elem, int n_control, bool has_grad_obs, bool has_grad_state, bool has_grad_reward) {
  const int64_t in = (int64_t)(2 * S + A) + (has_grad_obs ? O + n_control : 0) + (has_grad_state ? S : 0) + (has_grad_reward ? 1 + n_control : 0);
  return (int64_t)elem * (in + S + A);
}

}  // namespace excenv
