// Closed-loop rollouts: what excenv_sim_feedback and excenv_sim_policy have in common on the host. Host-only and free of HIP, like
// step_jac.hpp: the call record of both (feedback.hpp, policy.hpp name their instances) and the refusal both make about the clamp.
#pragma once
#include <cstdint>
#include <cstdio>
#include "../../include/excenv.h"

namespace excenv {

// The validated call (excenv_api.hip): K action rows of `substeps` solver steps each for B environments, every action computed inside
// the launch from the observation row saved at its start, by the controller that the policy record P describes (include/excenv.h
// excenv_feedback_t, excenv_policy_t).
template <class P> struct ClosedLoopCall {
  int solver, dtype;
  int64_t B, K;
  int32_t substeps;
  const excenv_props_t* props;
  const excenv_control_t* control;  // nullptr when n_control == 0
  double obs_stepsize, env_tau;     // the solver's step and the environment's tau (PMSM's dead-time advance)
  const void* const* state_in;      // S pointers
  const P* policy;
  void* obs_traj;                   // [N + 1][O + n_control][B]
  void* const* state_traj;          // S pointers to [N + 1][B], or nullptr
  void* const* last_state;          // S pointers to [B]
  void* actions_out;                // [K][A][B] or nullptr
  void* stream;                     // hipStream_t
};

// The clamp of a policy record must be an interval: EXCENV_OK, or EXCENV_EINVAL with the message in `msg`. A NaN bound fails `lo <= hi`.
inline int clip_refusal(const char* fn, double lo, double hi, char* msg, size_t n) {
  if (lo <= hi) return EXCENV_OK;
  std::snprintf(msg, n, "%s: policy->clip_lo = %g and policy->clip_hi = %g are not an interval (-inf / +inf: no clamp)", fn, lo, hi);
  return EXCENV_EINVAL;
}

}  // namespace excenv
