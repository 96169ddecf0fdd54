// Reverse mode of the reward of a stored trajectory: what one excenv_rew_vjp call launches. Host-only and free of HIP, like vjp.hpp:
// the call record, which state leaves the reward reads and the two forms of rew_vjp_kernel (kernels_rew_vjp.hpp).
#pragma once
#include "sim_plan.hpp"

namespace excenv {

// The validated call (excenv_api.hip): element strides as the caller gave them, outputs lane-major [rows][B]
struct RewVjpCall {
  int dtype;
  int64_t B, rows;
  const excenv_props_t* props;
  const excenv_control_t* control;      // nullptr when n_control == 0
  const int64_t* ref_strides;           // [n_control][2] element strides (env, row) of each reference array, or nullptr
  const void* const* state_traj;        // S pointers (read leaves non-NULL)
  int64_t s_sb, s_sk;                   // element strides (env, row) of every state leaf
  const void* grad_reward;              // rows - 1 values per environment, row n >= 1 at index n - 1
  int64_t g_sb, g_sk;
  void* const* grad_state_traj;         // S pointers: [rows][B] where the leaf is read, ignored elsewhere
  const uint8_t* reads;                 // reward_reads() of the call
  int V;                                // environments per lane: 1 (strided form) or 16 / elem (fast form)
  void* stream;                         // hipStream_t
};

// Which state leaves the reward reads (models.hpp env_reward / pmsm_reward): the controlled fields; PMSM: i_d, i_q when both are
// controlled (current reward), i_d, i_q, torque when torque is controlled (torque reward), nothing otherwise.
inline void reward_reads(int env, int n_control, const int32_t* control_idx, uint8_t (&reads)[EXCENV_MAX_STATE]) {
  for (int j = 0; j < EXCENV_MAX_STATE; ++j) reads[j] = 0;
  if (env == EXCENV_PMSM) {
    bool has_id = false, has_iq = false, has_tq = false;
    for (int j = 0; j < n_control; ++j) {
      has_id |= control_idx[j] == 3;
      has_iq |= control_idx[j] == 4;
      has_tq |= control_idx[j] == 5;
    }
    if ((has_id && has_iq) || has_tq) reads[3] = reads[4] = 1;
    if (has_tq) reads[5] = 1;
    return;
  }
  for (int j = 0; j < n_control; ++j)
    if (control_idx[j] >= 0 && control_idx[j] < EXCENV_MAX_STATE) reads[control_idx[j]] = 1;
}

// Environments per lane. The fast form (16 bytes per lane) needs `fast_ok`: lane-major state leaves, references and reward
// cotangent, B % (16 / elem) == 0, 16-byte aligned arrays, broadcast properties. `forced` is excenv_launch_opts_t.envs_per_lane
// (0: the fast form wherever it can be had). Returns 0 when a forced width cannot be had.
constexpr int rew_vjp_envs_per_lane(int elem, int forced, bool fast_ok) {
  const int vmax = 16 / elem;
  if (forced == 1) return 1;
  if (forced > 0) return (forced == vmax && fast_ok) ? vmax : 0;
  return fast_ok ? vmax : 1;
}

constexpr const char* rew_vjp_name(int V) {
  return V == 1 ? "rew_vjp_kernel (V=1, strided)" : V == 2 ? "rew_vjp_kernel (V=2)" : "rew_vjp_kernel (V=4)";
}

}  // namespace excenv
