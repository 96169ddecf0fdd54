// Closed-loop trajectories: what one excenv_sim_feedback call launches. Host-only and free of HIP, like step_jac.hpp: the call record,
// what the entry point refuses about the policy before any launch and the name of sim_feedback_kernel (kernels_feedback.hpp).
#pragma once
#include "closed_loop_call.hpp"

namespace excenv {

// The validated call (closed_loop_call.hpp) with the affine policy record (include/excenv.h excenv_feedback_t)
using FeedbackCall = ClosedLoopCall<excenv_feedback_t>;

// sim_feedback_kernel<M, T, SOLVER> exists for the seven models (the saturated PMSM included), the three solvers and both element
// types, one environment per lane: the only form, so excenv_launch_opts_t.envs_per_lane must be 0 (auto) or 1.
constexpr const char* feedback_name() { return "sim_feedback_kernel"; }

// What excenv_sim_feedback refuses about the policy record for a batch of B: EXCENV_OK, or the code with the message in `msg`.
// NULL pointers first, then values. A NaN bound fails `lo <= hi`.
inline int feedback_policy_refusal(const excenv_feedback_t* p, int64_t B, char* msg, size_t n) {
  const char* fn = "excenv_sim_feedback";
  if (!p) { std::snprintf(msg, n, "%s: policy is NULL", fn); return EXCENV_ENULL; }
  if (!p->gain) { std::snprintf(msg, n, "%s: policy->gain is NULL", fn); return EXCENV_ENULL; }
  if (p->integral_gain && !p->z_out) {
    std::snprintf(msg, n, "%s: policy->integral_gain without policy->z_out (the integrator state has to go somewhere)", fn);
    return EXCENV_ENULL;
  }
  if (p->gain_batch != 1 && p->gain_batch != B) {
    std::snprintf(msg, n, "%s: policy->gain_batch must be 1 (one gain set for all) or the batch size %lld (got %lld)", fn, (long long)B,
                  (long long)p->gain_batch);
    return EXCENV_EINVAL;
  }
  return clip_refusal(fn, p->clip_lo, p->clip_hi, msg, n);
}

}  // namespace excenv
