// Policy rollouts: what one excenv_sim_policy call launches. Host-only and free of HIP, like feedback.hpp: the call record, what the
// entry point refuses about the policy before any launch, the layout of the parameter array, the dynamic LDS of a launch and the
// name of sim_policy_kernel (kernels_policy.hpp). Below them the same for excenv_sim_policy_episodes: the call with its episode
// record, what the entry point refuses about that record, the name of sim_episodes_kernel (kernels_policy_episodes.hpp). Last the
// reverse mode, excenv_sim_policy_vjp: its call, its LDS and bytes, its refusals and the name of sim_policy_vjp_kernel
// (kernels_policy_vjp.hpp), and the parameter gradient, excenv_policy_param_grad: its tiles, workgroups, LDS, workspace and refusals
// (policy_param_grad.hip). Behind them the update step on stored rows: excenv_policy_eval (policy_eval.hip: tiles, workgroups, LDS,
// refusals), excenv_gae (gae.hip: block, prefetch depth, refusals) and the PPO objective, excenv_gaussian_logp / excenv_ppo_loss /
// excenv_ppo_loss_grad (ppo_loss.hip: tiles, workgroups, workspace, refusals).
#pragma once
#include "closed_loop_call.hpp"

namespace excenv {

// The validated call (closed_loop_call.hpp) with the MLP policy record (include/excenv.h excenv_policy_t)
using PolicyCall = ClosedLoopCall<excenv_policy_t>;

// sim_policy_kernel<M, T, SOLVER> exists for the seven models (the saturated PMSM included), the three solvers and both element
// types, one environment per lane: the only form, so excenv_launch_opts_t.envs_per_lane must be 0 (auto) or 1.
constexpr const char* policy_name() { return "sim_policy_kernel"; }

// One wavefront per workgroup: the kernel has no barrier, a lane only reads the LDS column it wrote, and the widest call (two
// ping-pong buffers of 64 fp64 activations per lane) then takes 64 KB of the CU's 160 KB, so two such workgroups still share a CU.
constexpr int POLICY_BLOCK = 64;

// The widest hidden layer of a validated policy (0 for L == 1), and the dynamic LDS of its launch: h[2][widest][POLICY_BLOCK]
inline int policy_widest_hidden(const excenv_policy_t& p) {
  int w = 0;
  for (int l = 1; l < p.n_layers; ++l) w = p.widths[l] > w ? p.widths[l] : w;
  return w;
}
inline size_t policy_lds_bytes(const excenv_policy_t& p, size_t elem) { return 2 * (size_t)policy_widest_hidden(p) * POLICY_BLOCK * elem; }

// The number of elements of `params`: for each layer W_l [d_l][d_{l-1}], then b_l [d_l]
inline int64_t policy_param_count(const excenv_policy_t& p) {
  int64_t n = 0;
  for (int l = 1; l <= p.n_layers; ++l) n += (int64_t)p.widths[l] * (p.widths[l - 1] + 1);
  return n;
}

// What excenv_sim_policy (and excenv_sim_policy_episodes, under its own name `fn`) refuses about the policy record for an environment of observation width OW and A actions: EXCENV_OK, or
// the code with the message in `msg`. NULL pointers first, then values. A NaN bound fails `lo <= hi`.
inline int policy_refusal(const excenv_policy_t* p, int OW, int A, char* msg, size_t n, const char* fn = "excenv_sim_policy") {
  if (!p) { std::snprintf(msg, n, "%s: policy is NULL", fn); return EXCENV_ENULL; }
  if (!p->params) { std::snprintf(msg, n, "%s: policy->params is NULL", fn); return EXCENV_ENULL; }
  if (p->n_layers < 1 || p->n_layers > EXCENV_POLICY_MAX_LAYERS) {
    std::snprintf(msg, n, "%s: policy->n_layers must be 1 .. %d (got %d)", fn, EXCENV_POLICY_MAX_LAYERS, p->n_layers);
    return EXCENV_EINVAL;
  }
  if (p->widths[0] != OW || p->widths[p->n_layers] != A) {
    std::snprintf(msg, n, "%s: policy->widths must run from the observation width %d to the action width %d (got %d .. %d)", fn, OW, A,
                  p->widths[0], p->widths[p->n_layers]);
    return EXCENV_EINVAL;
  }
  for (int l = 1; l < p->n_layers; ++l) {
    if (p->widths[l] < 1 || p->widths[l] > EXCENV_POLICY_MAX_WIDTH) {
      std::snprintf(msg, n, "%s: policy->widths[%d] must be 1 .. %d (got %d)", fn, l, EXCENV_POLICY_MAX_WIDTH, p->widths[l]);
      return EXCENV_EINVAL;
    }
  }
  if (p->activation != EXCENV_ACT_RELU && p->activation != EXCENV_ACT_TANH) {
    std::snprintf(msg, n, "%s: policy->activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got %d)", fn, p->activation);
    return EXCENV_EINVAL;
  }
  return clip_refusal(fn, p->clip_lo, p->clip_hi, msg, n);
}

// ---- episode rollouts: excenv_sim_policy_episodes ------------------------------------------------------------------
// The validated call: a policy call with the episode record (include/excenv.h excenv_episode_t)
struct EpisodeCall {
  PolicyCall call;
  const excenv_episode_t* episode;
};

// sim_episodes_kernel<M, T, SOLVER> (kernels_policy_episodes.hpp): the same 42 instantiations, one environment per lane
constexpr const char* episodes_name() { return "sim_episodes_kernel"; }

// What excenv_sim_policy_episodes refuses about the episode record of a model with S state fields, behind every check of
// excenv_sim_policy: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values.
inline int episode_refusal(const excenv_episode_t* e, int S, int32_t substeps, char* msg, size_t n) {
  const char* fn = "excenv_sim_policy_episodes";
  if (!e) { std::snprintf(msg, n, "%s: episode is NULL", fn); return EXCENV_ENULL; }
  if (!e->reset_states) { std::snprintf(msg, n, "%s: episode->reset_states is NULL", fn); return EXCENV_ENULL; }
  for (int j = 0; j < S; ++j)
    if (!e->reset_states[j]) { std::snprintf(msg, n, "%s: episode->reset_states pointer %d is NULL", fn, j); return EXCENV_ENULL; }
  if (substeps != 1) {
    std::snprintf(msg, n, "%s: substeps must be 1 (one solver step per action, as GymWrapper.step does; got %d)", fn, substeps);
    return EXCENV_EINVAL;
  }
  if (e->n_reset_rows < 1) {
    std::snprintf(msg, n, "%s: episode->n_reset_rows must be at least 1 (got %d)", fn, e->n_reset_rows);
    return EXCENV_EINVAL;
  }
  if (e->end_mask & ~(EXCENV_END_TERMINATED | EXCENV_END_TRUNCATED)) {
    std::snprintf(msg, n, "%s: episode->end_mask has unknown bits (got %d; EXCENV_END_TERMINATED = 1, EXCENV_END_TRUNCATED = 2)", fn,
                  e->end_mask);
    return EXCENV_EINVAL;
  }
  if (e->max_episode_steps < 0) {
    std::snprintf(msg, n, "%s: episode->max_episode_steps must not be negative (got %d; 0: no time limit)", fn, e->max_episode_steps);
    return EXCENV_EINVAL;
  }
  if (e->end_mask == 0 && e->max_episode_steps == 0) {
    std::snprintf(msg, n, "%s: episode->end_mask = 0 and episode->max_episode_steps = 0: nothing can end an episode (use excenv_sim_policy)", fn);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

// ---- reverse mode of the policy rollout: excenv_sim_policy_vjp -----------------------------------------------------
// The validated call: the stored forward of one excenv_sim_policy (or excenv_sim_policy_episodes) call, the cotangents of its outputs
// and where the gradients go (include/excenv.h excenv_policy_vjp_t). Everything lane-major.
struct PolicyVjpCall {
  int solver, dtype;
  int64_t B, K;
  int32_t substeps;
  const excenv_props_t* props;
  const excenv_control_t* control;  // nullptr when n_control == 0; only n_control is read (references get no gradient)
  double obs_stepsize, env_tau;
  const excenv_policy_vjp_t* r;
  void* stream;  // hipStream_t
};

// sim_policy_vjp_kernel<M, T, SOLVER> (kernels_policy_vjp.hpp): six models (no saturated PMSM), three solvers, both element types
constexpr const char* policy_vjp_name() { return "sim_policy_vjp_kernel"; }

// The dynamic LDS of its launch: every hidden layer of the lane's column at once, h[d_1 + .. + d_{L-1}][POLICY_BLOCK] (0 for L == 1);
// at most 3 * 64 rows: 48 KB (fp32) / 96 KB (fp64)
inline size_t policy_vjp_lds_bytes(const excenv_policy_t& p, size_t elem) {
  size_t rows = 0;
  for (int l = 1; l < p.n_layers; ++l) rows += (size_t)p.widths[l];
  return rows * POLICY_BLOCK * elem;
}

// Algorithmic bytes per environment and action row of the reverse launch, w = elem: per solver step the saved row
// (S) and the cotangent rows that are present (O of grad_obs: the control columns are skipped; S of grad_states); per action row the
// stored observation row (OW), the applied action (A), grad_actions (A, present) in and grad_raw (A) out; one byte of the episode mask
constexpr int64_t policy_vjp_bytes(int S, int A, int O, int elem, int n_control, int32_t substeps, bool has_grad_obs, bool has_grad_states,
                                   bool has_grad_actions, bool has_reset) {
  return (int64_t)elem * ((int64_t)substeps * (S + (has_grad_obs ? O : 0) + (has_grad_states ? S : 0)) + (O + n_control) +
                          A * (2 + (has_grad_actions ? 1 : 0))) + (has_reset ? 1 : 0);
}

// What excenv_sim_policy_vjp refuses about its record for K action rows of `substeps` steps, behind excenv_sim_policy's checks of
// the policy inside it: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values.
inline int policy_vjp_refusal(const excenv_policy_vjp_t* r, int64_t K, int32_t substeps, char* msg, size_t n) {
  const char* fn = "excenv_sim_policy_vjp";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!r->obs_traj) return null("call->obs_traj (the policy is evaluated again on the saved observation rows)");
  if (!r->state_traj) return null("call->state_traj (the reverse pass reads the saved rows)");
  if (K > 0 && !r->actions) return null("call->actions");
  if (!r->grad_state0) return null("call->grad_state0");
  if (K > 0 && !r->grad_raw) return null("call->grad_raw");
  if (r->reset && substeps != 1) {
    std::snprintf(msg, n, "%s: call->reset needs substeps == 1 (one solver step per action, as excenv_sim_policy_episodes; got %d)", fn, substeps);
    return EXCENV_EINVAL;
  }
  if (K > (int64_t)0x7fffffff / substeps) {
    std::snprintf(msg, n, "%s: K * substeps = %lld * %d rows exceed one launch", fn, (long long)K, (int)substeps);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

// ---- the parameter gradient of a policy rollout: excenv_policy_param_grad ------------------------------------------
// policy_param_grad_kernel<T> and policy_param_grad_reduce_kernel<T> (policy_param_grad.hip): no model, one instantiation per type
constexpr const char* policy_param_grad_name() { return "policy_param_grad_kernel"; }

constexpr int PARAM_GRAD_BLOCK = 256;  // four waves
constexpr int PARAM_GRAD_TILE = 64;    // samples of one tile: 64 consecutive environments of one action row
// The row stride of the tile in LDS, in elements: 2 mod 32, so that the sixteen rows j0 + (l & 15) at the two columns s0 + (l >> 4) of
// a 32-lane group (the operand reads of the weight product) fall on 32 different banks, in 4-byte and in 8-byte elements
constexpr int PARAM_GRAD_LDS_STRIDE = PARAM_GRAD_TILE + 2;
// 16 x 16 output tiles of the weight product a wave holds in registers: the widest network has 8 + 20 + 20 + 5 = 53 over four waves
constexpr int PARAM_GRAD_SLOTS = 14;

// The rows of the tile in LDS: x^0 (OW), every hidden x^l (d^l over it in place), d^L (A) and the ones row of the bias sums
inline int policy_param_grad_lds_rows(const excenv_policy_t& p) {
  int rows = p.widths[0] + p.widths[p.n_layers] + 1;
  for (int l = 1; l < p.n_layers; ++l) rows += p.widths[l];
  return rows;
}
inline size_t policy_param_grad_lds_bytes(const excenv_policy_t& p, size_t elem) {
  return (size_t)policy_param_grad_lds_rows(p) * PARAM_GRAD_LDS_STRIDE * elem;
}
// 16 x 16 output tiles of all the weight products: per layer ceil(d_l / 16) x ceil((d_{l-1} + 1) / 16), the bias as one more column
inline int policy_param_grad_out_tiles(const excenv_policy_t& p) {
  int n = 0;
  for (int l = 1; l <= p.n_layers; ++l) n += ((p.widths[l] + 15) / 16) * ((p.widths[l - 1] + 1 + 15) / 16);
  return n;
}

// Sample tiles of a call, its workgroups and the first tile of workgroup g (g == groups: one past the last tile): functions of
// (B, K, max_groups) only
inline int64_t policy_param_grad_tiles(int64_t B, int64_t K) { return K * ((B + PARAM_GRAD_TILE - 1) / PARAM_GRAD_TILE); }
inline int64_t policy_param_grad_groups(int64_t B, int64_t K, int32_t max_groups) {
  const int64_t tiles = policy_param_grad_tiles(B, K), cap = max_groups > 0 ? max_groups : EXCENV_PARAM_GRAD_AUTO_GROUPS;
  return tiles < cap ? tiles : cap;
}
// (every workgroup gets floor(tiles / groups) tiles, the first tiles % groups of them one more)
inline int64_t policy_param_grad_first_tile(int64_t tiles, int64_t groups, int64_t g) {
  const int64_t q = tiles / groups, r = tiles % groups;
  return g * q + (g < r ? g : r);
}
inline int64_t policy_param_grad_workspace(int64_t B, int64_t K, const excenv_policy_t& p, int32_t max_groups) {
  return policy_param_grad_groups(B, K, max_groups) * policy_param_count(p) * 8;
}

// What excenv_policy_param_grad refuses: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values.
inline int policy_param_grad_refusal(int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_policy_param_grad_t* c, char* msg,
                                     size_t n) {
  const char* fn = "excenv_policy_param_grad";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  const excenv_policy_t& p = c->policy;
  if (!p.params) return null("call->policy.params");
  if (!c->obs_traj) return null("call->obs_traj");
  if (K > 0 && !c->grad_raw) return null("call->grad_raw");
  if (!c->grad_params) return null("call->grad_params");
  if (!c->workspace) return null("call->workspace");
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) {
    std::snprintf(msg, n, "%s: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got %d)", fn, dtype);
    return EXCENV_EINVAL;
  }
  if (B < 0 || K < 0 || substeps < 1) {
    std::snprintf(msg, n, "%s: bad B=%lld, K=%lld or substeps=%d", fn, (long long)B, (long long)K, (int)substeps);
    return EXCENV_EINVAL;
  }
  if (K > (int64_t)0x7fffffff / substeps) {
    std::snprintf(msg, n, "%s: K * substeps = %lld * %d rows exceed one launch", fn, (long long)K, (int)substeps);
    return EXCENV_EINVAL;
  }
  if (p.n_layers < 1 || p.n_layers > EXCENV_POLICY_MAX_LAYERS) {
    std::snprintf(msg, n, "%s: policy.n_layers must be 1 .. %d (got %d)", fn, EXCENV_POLICY_MAX_LAYERS, p.n_layers);
    return EXCENV_EINVAL;
  }
  for (int l = 1; l < p.n_layers; ++l) {
    if (p.widths[l] < 1 || p.widths[l] > EXCENV_POLICY_MAX_WIDTH) {
      std::snprintf(msg, n, "%s: policy.widths[%d] must be 1 .. %d (got %d)", fn, l, EXCENV_POLICY_MAX_WIDTH, p.widths[l]);
      return EXCENV_EINVAL;
    }
  }
  if (p.widths[0] < 1 || p.widths[0] > EXCENV_POLICY_MAX_INPUT) {
    std::snprintf(msg, n, "%s: policy.widths[0] must be 1 .. %d (the widest observation row; got %d)", fn, EXCENV_POLICY_MAX_INPUT, p.widths[0]);
    return EXCENV_EINVAL;
  }
  if (p.widths[p.n_layers] < 1 || p.widths[p.n_layers] > EXCENV_MAX_ACTION) {
    std::snprintf(msg, n, "%s: policy.widths[%d] must be 1 .. %d (the action width; got %d)", fn, p.n_layers, EXCENV_MAX_ACTION,
                  p.widths[p.n_layers]);
    return EXCENV_EINVAL;
  }
  if (p.activation != EXCENV_ACT_RELU && p.activation != EXCENV_ACT_TANH) {
    std::snprintf(msg, n, "%s: policy.activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got %d)", fn, p.activation);
    return EXCENV_EINVAL;
  }
  if (c->max_groups < 0) {
    std::snprintf(msg, n, "%s: call->max_groups must not be negative (got %d; 0: auto)", fn, c->max_groups);
    return EXCENV_EINVAL;
  }
  const int64_t need = policy_param_grad_workspace(B, K, p, c->max_groups);
  if (c->workspace_bytes < need || (reinterpret_cast<uintptr_t>(c->workspace) & 7u) != 0) {
    std::snprintf(msg, n, "%s: needs an 8-byte aligned workspace of %lld bytes (excenv_policy_param_grad_workspace_bytes)", fn, (long long)need);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

// ---- the network on stored rows: excenv_policy_eval ----------------------------------------------------------------
// policy_eval_kernel<T> (policy_eval.hip): no model, one instantiation per type
constexpr const char* policy_eval_name() { return "policy_eval_kernel"; }

// Whether the fp64 instantiation multiplies on the matrix cores (v_mfma_f64_16x16x4_f64) or by per-lane fma chains; the fp32 one
// always uses v_mfma_f32_16x16x4_f32. The contract is the bits of the chain either way (DESIGN.md §4.17 says which form shipped).
constexpr bool POLICY_EVAL_F64_MMA = true;
// Workgroups of a launch at the most: eight for each of the 256 compute units
constexpr int POLICY_EVAL_MAX_GROUPS = 2048;

// The rows of the tile in LDS, PARAM_GRAD_LDS_STRIDE elements each: x^0 twice (the next tile is staged while this one is read), then
// two buffers the hidden layers alternate between: x^1 and x^3 in the first, x^2 in the second
inline int policy_eval_lds_rows(const excenv_policy_t& p) {
  const int L = p.n_layers;
  const int h1 = L >= 2 ? p.widths[1] : 0, h2 = L >= 3 ? p.widths[2] : 0, h3 = L >= 4 ? p.widths[3] : 0;
  return 2 * p.widths[0] + (h1 > h3 ? h1 : h3) + h2;
}
inline size_t policy_eval_lds_bytes(const excenv_policy_t& p, size_t elem) {
  return (size_t)policy_eval_lds_rows(p) * PARAM_GRAD_LDS_STRIDE * elem;
}

// Sample tiles of a call (64 consecutive environments of one evaluated row, tile number r * ceil(B / 64) + b_tile) and its workgroups;
// workgroup g owns the tiles policy_param_grad_first_tile(tiles, groups, g) .. (g + 1) - 1: functions of (B, R) only
inline int64_t policy_eval_tiles(int64_t B, int64_t R) { return R * ((B + PARAM_GRAD_TILE - 1) / PARAM_GRAD_TILE); }
inline int64_t policy_eval_groups(int64_t B, int64_t R) {
  const int64_t tiles = policy_eval_tiles(B, R);
  return tiles < POLICY_EVAL_MAX_GROUPS ? tiles : POLICY_EVAL_MAX_GROUPS;
}

// What excenv_policy_eval refuses: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values.
inline int policy_eval_refusal(int dtype, int64_t B, int64_t R, int64_t row_stride, const excenv_policy_eval_t* c, char* msg, size_t n) {
  const char* fn = "excenv_policy_eval";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  const excenv_policy_t& p = c->policy;
  if (!p.params) return null("call->policy.params");
  if (!c->obs_traj) return null("call->obs_traj");
  if (!c->out) return null("call->out");
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) {
    std::snprintf(msg, n, "%s: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got %d)", fn, dtype);
    return EXCENV_EINVAL;
  }
  if (B < 0 || R < 0 || row_stride < 1) {
    std::snprintf(msg, n, "%s: bad B=%lld, R=%lld or row_stride=%lld", fn, (long long)B, (long long)R, (long long)row_stride);
    return EXCENV_EINVAL;
  }
  if (R > 1 && row_stride > (int64_t)0x7fffffff / (R - 1)) {
    std::snprintf(msg, n, "%s: (R - 1) * row_stride = %lld * %lld rows exceed one launch", fn, (long long)(R - 1), (long long)row_stride);
    return EXCENV_EINVAL;
  }
  if (p.n_layers < 1 || p.n_layers > EXCENV_POLICY_MAX_LAYERS) {
    std::snprintf(msg, n, "%s: policy.n_layers must be 1 .. %d (got %d)", fn, EXCENV_POLICY_MAX_LAYERS, p.n_layers);
    return EXCENV_EINVAL;
  }
  for (int l = 1; l < p.n_layers; ++l) {
    if (p.widths[l] < 1 || p.widths[l] > EXCENV_POLICY_MAX_WIDTH) {
      std::snprintf(msg, n, "%s: policy.widths[%d] must be 1 .. %d (got %d)", fn, l, EXCENV_POLICY_MAX_WIDTH, p.widths[l]);
      return EXCENV_EINVAL;
    }
  }
  if (p.widths[0] < 1 || p.widths[0] > EXCENV_POLICY_MAX_INPUT) {
    std::snprintf(msg, n, "%s: policy.widths[0] must be 1 .. %d (the widest observation row; got %d)", fn, EXCENV_POLICY_MAX_INPUT, p.widths[0]);
    return EXCENV_EINVAL;
  }
  if (p.widths[p.n_layers] < 1 || p.widths[p.n_layers] > EXCENV_MAX_ACTION) {
    std::snprintf(msg, n, "%s: policy.widths[%d] must be 1 .. %d (the action width; got %d)", fn, p.n_layers, EXCENV_MAX_ACTION,
                  p.widths[p.n_layers]);
    return EXCENV_EINVAL;
  }
  if (p.activation != EXCENV_ACT_RELU && p.activation != EXCENV_ACT_TANH) {
    std::snprintf(msg, n, "%s: policy.activation must be EXCENV_ACT_RELU (0) or EXCENV_ACT_TANH (1) (got %d)", fn, p.activation);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

// ---- generalised advantage estimation on lane-major rows: excenv_gae ----------------------------------------------
// gae_kernel<T> (gae.hip): one environment per lane, one instantiation per type
constexpr const char* gae_name() { return "gae_kernel"; }
constexpr int GAE_BLOCK = 256;
// Rows of loads a lane keeps in flight ahead of the scan (the loads of row n do not depend on the carry)
constexpr int GAE_DEPTH = 8;

// What excenv_gae refuses: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values. A NaN fails both
// comparisons of its range.
inline int gae_refusal(int dtype, int64_t B, int64_t K, const excenv_gae_t* c, char* msg, size_t n) {
  const char* fn = "excenv_gae";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  if (!c->reward) return null("call->reward");
  if (!c->value) return null("call->value");
  if (!c->advantage) return null("call->advantage");
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) {
    std::snprintf(msg, n, "%s: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got %d)", fn, dtype);
    return EXCENV_EINVAL;
  }
  if (B < 0 || K < 0) {
    std::snprintf(msg, n, "%s: bad B=%lld or K=%lld", fn, (long long)B, (long long)K);
    return EXCENV_EINVAL;
  }
  if (!(c->gamma >= 0.0 && c->gamma <= 1.0)) {
    std::snprintf(msg, n, "%s: call->gamma must lie in [0, 1] (got %g)", fn, c->gamma);
    return EXCENV_EINVAL;
  }
  if (!(c->lambda >= 0.0 && c->lambda <= 1.0)) {
    std::snprintf(msg, n, "%s: call->lambda must lie in [0, 1] (got %g)", fn, c->lambda);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

// ---- the clipped PPO objective on lane-major rows: excenv_gaussian_logp, excenv_ppo_loss, excenv_ppo_loss_grad -----
// gaussian_logp_kernel<T, A>, ppo_loss_kernel<T, A>, ppo_loss_grad_kernel<T, A> and ppo_loss_reduce_kernel (ppo_loss.hip): no model,
// one instantiation per type and action width
constexpr const char* gaussian_logp_name() { return "gaussian_logp_kernel"; }
constexpr const char* ppo_loss_name() { return "ppo_loss_kernel"; }
constexpr const char* ppo_loss_grad_name() { return "ppo_loss_grad_kernel"; }
constexpr int PPO_BLOCK = 256;                           // four waves
constexpr int PPO_LANE = EXCENV_PPO_TILE / PPO_BLOCK;    // consecutive samples of a lane: 16 bytes of fp32
static_assert(PPO_LANE == 4, "a lane's samples are one 16-byte access in fp32, two in fp64");
constexpr int PPO_SLOTS = EXCENV_PPO_STATS + EXCENV_MAX_ACTION;  // fp64 sums of one partial set

// Sample tiles of a call (EXCENV_PPO_TILE consecutive environments of one row, tile number n * ceil(B / EXCENV_PPO_TILE) + b_tile) and
// its workgroups; workgroup g owns the tiles policy_param_grad_first_tile(tiles, groups, g) .. (g + 1) - 1: functions of
// (B, K, max_groups) only
inline int64_t ppo_tiles(int64_t B, int64_t K) { return K * ((B + EXCENV_PPO_TILE - 1) / EXCENV_PPO_TILE); }
inline int64_t ppo_groups(int64_t B, int64_t K, int32_t max_groups) {
  const int64_t tiles = ppo_tiles(B, K), cap = max_groups > 0 ? max_groups : EXCENV_PPO_AUTO_GROUPS;
  return tiles < cap ? tiles : cap;
}
inline int64_t ppo_loss_workspace(int64_t B, int64_t K, int32_t max_groups) { return ppo_groups(B, K, max_groups) * PPO_SLOTS * 8; }

// What the three entries refuse: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values. A NaN fails both
// comparisons of clip_eps' range.
inline int ppo_common_refusal(const char* fn, int n_actions, int dtype, int64_t B, int64_t K, char* msg, size_t n) {
  if (n_actions < 1 || n_actions > EXCENV_MAX_ACTION) {
    std::snprintf(msg, n, "%s: call->n_actions must be 1 .. %d (got %d)", fn, EXCENV_MAX_ACTION, n_actions);
    return EXCENV_EINVAL;
  }
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) {
    std::snprintf(msg, n, "%s: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got %d)", fn, dtype);
    return EXCENV_EINVAL;
  }
  if (B < 0 || K < 0) {
    std::snprintf(msg, n, "%s: bad B=%lld or K=%lld", fn, (long long)B, (long long)K);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}
inline int ppo_rows_refusal(const char* fn, int n_actions, int64_t K, char* msg, size_t n) {
  if (K > (int64_t)0x7fffffff / n_actions) {
    std::snprintf(msg, n, "%s: K * n_actions = %lld * %d rows exceed one launch", fn, (long long)K, n_actions);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}
inline int gaussian_logp_refusal(int dtype, int64_t B, int64_t K, const excenv_gaussian_logp_t* c, char* msg, size_t n) {
  const char* fn = "excenv_gaussian_logp";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  if (!c->mean) return null("call->mean");
  if (!c->sample) return null("call->sample");
  if (!c->inv_std) return null("call->inv_std");
  if (!c->logp_const) return null("call->logp_const");
  if (!c->logp) return null("call->logp");
  if (int rc = ppo_common_refusal(fn, c->n_actions, dtype, B, K, msg, n)) return rc;
  return ppo_rows_refusal(fn, c->n_actions, K, msg, n);
}
// grad: excenv_ppo_loss_grad (grad_scale and an output instead of stats and the workspace)
inline int ppo_loss_refusal(bool grad, int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t* c, char* msg, size_t n) {
  const char* fn = grad ? "excenv_ppo_loss_grad" : "excenv_ppo_loss";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  if (!c->mean) return null("call->mean");
  if (!c->sample) return null("call->sample");
  if (!c->inv_std) return null("call->inv_std");
  if (!c->logp_const) return null("call->logp_const");
  if (!c->logp_old) return null("call->logp_old");
  if (!c->advantage) return null("call->advantage");
  if (grad) {
    if (!c->grad_scale) return null("call->grad_scale");
    if (!c->grad_mean && !c->grad_value) return null("call->grad_mean and call->grad_value");
  } else {
    if (!c->stats) return null("call->stats");
    if (!c->workspace) return null("call->workspace");
  }
  if ((c->value != nullptr) != (c->returns != nullptr)) {
    std::snprintf(msg, n, "%s: call->value and call->returns must be given both or neither", fn);
    return EXCENV_EINVAL;
  }
  if (grad && c->grad_value && !c->value) {
    std::snprintf(msg, n, "%s: call->grad_value needs call->value and call->returns", fn);
    return EXCENV_EINVAL;
  }
  if (int rc = ppo_common_refusal(fn, c->n_actions, dtype, B, K, msg, n)) return rc;
  if (!(c->clip_eps > 0.0 && c->clip_eps < 1.0)) {
    std::snprintf(msg, n, "%s: call->clip_eps must lie in (0, 1) (got %g)", fn, c->clip_eps);
    return EXCENV_EINVAL;
  }
  if (!grad) {
    if (c->max_groups < 0) {
      std::snprintf(msg, n, "%s: call->max_groups must not be negative (got %d; 0: auto)", fn, c->max_groups);
      return EXCENV_EINVAL;
    }
    const int64_t need = ppo_loss_workspace(B, K, c->max_groups);
    if (c->workspace_bytes < need || (reinterpret_cast<uintptr_t>(c->workspace) & 7u) != 0) {
      std::snprintf(msg, n, "%s: needs an 8-byte aligned workspace of %lld bytes (excenv_ppo_loss_workspace_bytes)", fn, (long long)need);
      return EXCENV_EINVAL;
    }
  }
  return ppo_rows_refusal(fn, c->n_actions, K, msg, n);
}

}  // namespace excenv
