// Reverse mode of the closed-loop trajectory: what one excenv_sim_feedback_vjp call launches. Host-only and free of HIP, like
// feedback.hpp and step_vjp.hpp: the call record, what the entry point refuses about the call record before any launch, the workspace
// layout, the algorithmic bytes and the name of sim_feedback_vjp_kernel (kernels_feedback_vjp.hpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include "vjp.hpp"

namespace excenv {

// The validated call (excenv_api.hip): the stored forward of one excenv_sim_feedback call, the cotangents of its outputs, and where
// the gradients go (include/excenv.h excenv_feedback_vjp_t). Everything lane-major.
struct FeedbackVjpCall {
  int solver, dtype;
  int64_t B, K;
  int32_t substeps;
  const excenv_props_t* props;
  const excenv_control_t* control;  // nullptr when n_control == 0; only n_control is read (references get no gradient)
  double obs_stepsize, env_tau;
  const excenv_feedback_vjp_t* r;
  void* workspace;
  void* stream;  // hipStream_t
};

constexpr const char* feedback_vjp_name() { return "sim_feedback_vjp_kernel"; }

// ---- the workspace, in this order (every part aligned like vjp.hpp's) ----------------------------------------------------------------
//   z rows     [K][A][B] elements: z_1 .. z_K of feedback_z_rows_kernel, with integral action only
//   gain terms [1 or 2][A][OW][B] elements: the per-environment gain gradients of a broadcast gain set (gain_batch == 1), which the
//              deterministic batch sum (param_sum.hip) then adds up; the second set with integral action
//   partials   the batch sum's own workspace for EXCENV_MAX_STATIC leaves: one call of it per chunk of that many gain entries
constexpr int64_t feedback_vjp_z_bytes(int A, int elem, int64_t B, int64_t K, bool integral) { return integral ? align_up(elem * K * A * B) : 0; }
constexpr int64_t feedback_vjp_terms_bytes(int A, int OW, int elem, int64_t B, int64_t gain_batch, bool integral) {
  return gain_batch == 1 ? align_up((int64_t)elem * (integral ? 2 : 1) * A * OW * B) : 0;
}
constexpr int64_t feedback_vjp_workspace_bytes(int A, int OW, int elem, int64_t B, int64_t K, int64_t gain_batch, bool integral) {
  return feedback_vjp_z_bytes(A, elem, B, K, integral) + feedback_vjp_terms_bytes(A, OW, elem, B, gain_batch, integral) +
         (gain_batch == 1 ? param_sum_workspace_bytes(B, EXCENV_MAX_STATIC) : 0);
}

// Algorithmic bytes per environment and action row of the whole backward launch sequence, w = elem:
//   reverse kernel: per solver step the saved row (S) and the cotangent rows that are present (O of grad_obs: the control columns are
//                   skipped; S of grad_states); per action row the applied action (A), z (A, integral), grad_actions (A, present) in,
//                   grad_ff (A) and grad_zi (A, integral) out
//   pre-pass      : OW observation columns in, A out (integral)
//   gain kernel   : OW observation columns and the grad_ff (grad_zi) row in, once per gain set
constexpr int64_t feedback_vjp_bytes(int S, int A, int O, int elem, int n_control, int32_t substeps, bool integral, bool has_grad_obs,
                                     bool has_grad_states, bool has_grad_actions) {
  const int64_t OW = O + n_control, sets = integral ? 2 : 1;
  const int64_t reverse = (int64_t)substeps * (S + (has_grad_obs ? O : 0) + (has_grad_states ? S : 0)) + A * (sets + (has_grad_actions ? 1 : 0)) + A * sets;
  const int64_t prepass = integral ? OW + A : 0;
  const int64_t gains = sets * (OW + A);
  return (int64_t)elem * (reverse + prepass + gains);
}

// What excenv_sim_feedback_vjp refuses about the call record for a batch of B and K action rows: EXCENV_OK, or the code with the
// message in `msg`. NULL pointers first, then values. A NaN bound fails `lo <= hi`.
inline int feedback_vjp_refusal(const excenv_feedback_vjp_t* r, int64_t B, int64_t K, char* msg, size_t n) {
  const char* fn = "excenv_sim_feedback_vjp";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!r) return null("call");
  if (!r->gain) return null("call->gain");
  if (!r->state_traj) return null("call->state_traj (the reverse pass reads the saved rows)");
  if (!r->obs_traj) return null("call->obs_traj (the gain gradients read the saved observation rows)");
  if (K > 0 && !r->actions) return null("call->actions");
  if (!r->grad_state0) return null("call->grad_state0");
  if (K > 0 && !r->grad_ff) return null("call->grad_ff (the gain gradients read it)");
  if (r->integral_gain && K > 0 && !r->grad_zi) return null("call->grad_zi (with integral_gain; the gain gradients read it)");
  if (r->integral_gain && !r->grad_z0) return null("call->grad_z0 (with integral_gain)");
  if (r->grad_integral_gain && !r->integral_gain) return null("call->integral_gain (with grad_integral_gain)");
  if (r->gain_batch != 1 && r->gain_batch != B) {
    std::snprintf(msg, n, "%s: call->gain_batch must be 1 (one gain set for all) or the batch size %lld (got %lld)", fn, (long long)B,
                  (long long)r->gain_batch);
    return EXCENV_EINVAL;
  }
  if (!(r->clip_lo <= r->clip_hi)) {
    std::snprintf(msg, n, "%s: call->clip_lo = %g and call->clip_hi = %g are not an interval (-inf / +inf: no clamp)", fn, r->clip_lo,
                  r->clip_hi);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

}  // namespace excenv
