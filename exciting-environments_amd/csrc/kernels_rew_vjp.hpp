// Reverse mode of generate_rew_trunc_term_ahead's reward on a stored trajectory (traj_gym_kernel, kernels.hpp): the transposed
// env_reward / pmsm_reward (models.hpp env_reward_vjp) at every saved row. Reads the state leaves the reward reads, the references of
// the controlled fields and the reward cotangent (row n >= 1 at index n - 1); writes one lane-major [rows][B] cotangent array per read
// leaf — the rows excenv_sim_ahead_vjp takes as grad_state_traj. Row 0 is written as zeros (the reward covers rows 1..).
// Two forms, the same device function and the same bits:
//   V = 16 / sizeof(T) (fast): a lane owns V adjacent environments of one row; everything lane-major, broadcast properties, 16-byte
//     loads and non-temporal 16-byte stores;
//   V = 1 (strided): one element per lane, any element strides on the inputs, per-environment property arrays; outputs lane-major.
// No LDS, no scratch. Instantiated in rew_vjp.hip only.
#pragma once
#include "launch.hpp"
#include "rew_vjp.hpp"

namespace excenv {

template <typename T, class M> struct RewVjpArgs {
  KProps<T, M> kp;
  int64_t B, rows;
  int32_t n_control;
  int32_t control_idx[EXCENV_MAX_CONTROL];
  const T* reference[EXCENV_MAX_CONTROL];
  int64_t r_sb[EXCENV_MAX_CONTROL], r_sk[EXCENV_MAX_CONTROL];
  const T* straj[M::S];  // nullptr where the leaf is not read
  int64_t s_sb, s_sk;
  const T* grad_reward;
  int64_t g_sb, g_sk;
  T* grad[M::S];         // [rows][B]; nullptr where the leaf is not read
};

template <class M, typename T, int V> __global__ void __launch_bounds__(BLOCK) rew_vjp_kernel(const RewVjpArgs<T, M> ka) {
  constexpr int S = M::S;
  const int64_t lanes = (ka.B + V - 1) / V;
  const int64_t nb = (lanes + BLOCK - 1) / BLOCK;
  const int64_t n = (int64_t)blockIdx.x / nb;  // row
  const int64_t lane = ((int64_t)blockIdx.x - n * nb) * BLOCK + threadIdx.x;
  const int64_t b0 = lane * V;  // first environment of the lane (V > 1: B % V == 0, the lane's V environments all exist)
  if (b0 >= ka.B || n >= ka.rows) return;
  T out[S][V];
#pragma unroll
  for (int j = 0; j < S; ++j)
#pragma unroll
    for (int v = 0; v < V; ++v) out[j][v] = T(0);
  if (n > 0) {
    Ctx<T, M> c;
    load_ctx<V == 1, T, M, false>(c, ka.kp, b0, T(0), T(0), T(0));
    T sv[S][V], rv[EXCENV_MAX_CONTROL][V], g[V];
#pragma unroll
    for (int j = 0; j < S; ++j) {
#pragma unroll
      for (int v = 0; v < V; ++v) sv[j][v] = T(0);
      if (ka.straj[j] != nullptr) load_v<T, V>(ka.straj[j] + b0 * ka.s_sb + n * ka.s_sk, sv[j]);  // V > 1: s_sb == 1
    }
#pragma unroll
    for (int j = 0; j < EXCENV_MAX_CONTROL; ++j) {
#pragma unroll
      for (int v = 0; v < V; ++v) rv[j][v] = T(0);
      if (j < ka.n_control) load_v<T, V>(ka.reference[j] + b0 * ka.r_sb[j] + n * ka.r_sk[j], rv[j]);  // V > 1: r_sb == 1
    }
    load_v<T, V>(ka.grad_reward + b0 * ka.g_sb + (n - 1) * ka.g_sk, g);  // V > 1: g_sb == 1
#pragma unroll
    for (int v = 0; v < V; ++v) {
      T st[S], gs[S], rref[EXCENV_MAX_CONTROL];
#pragma unroll
      for (int j = 0; j < S; ++j) {
        st[j] = sv[j][v];
        gs[j] = T(0);
      }
#pragma unroll
      for (int j = 0; j < EXCENV_MAX_CONTROL; ++j) rref[j] = rv[j][v];
      env_reward_vjp<M, T>(st, c, ka.n_control, ka.control_idx, rref, g[v], gs);
#pragma unroll
      for (int j = 0; j < S; ++j) out[j][v] = gs[j];
    }
  }
#pragma unroll
  for (int j = 0; j < S; ++j)
    if (ka.grad[j] != nullptr) store_stream<T, V>(ka.grad[j] + n * ka.B + b0, out[j]);
}

template <class M, typename T> static int launch_rew_vjp(const RewVjpCall& rc) {
  RewVjpArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, rc.props);
  ka.B = rc.B;
  ka.rows = rc.rows;
  ka.n_control = rc.control ? rc.control->n_control : 0;
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = rc.control->control_idx[j];
    ka.reference[j] = (const T*)rc.control->reference[j];
    ka.r_sb[j] = rc.ref_strides ? rc.ref_strides[2 * j] : 1;
    ka.r_sk[j] = rc.ref_strides ? rc.ref_strides[2 * j + 1] : 0;
  }
  for (int j = 0; j < M::S; ++j) {
    ka.straj[j] = rc.reads[j] ? (const T*)rc.state_traj[j] : nullptr;
    ka.grad[j] = rc.reads[j] ? (T*)rc.grad_state_traj[j] : nullptr;
  }
  ka.s_sb = rc.s_sb;
  ka.s_sk = rc.s_sk;
  ka.grad_reward = (const T*)rc.grad_reward;
  ka.g_sb = rc.g_sb;
  ka.g_sk = rc.g_sk;
  constexpr int VMAX = 16 / (int)sizeof(T);
  const int64_t lanes = (rc.B + rc.V - 1) / rc.V;
  const int64_t blocks = ((lanes + BLOCK - 1) / BLOCK) * rc.rows;
  if (blocks >= ((int64_t)1 << 31)) { set_error("excenv_rew_vjp: trajectory too large for one launch"); return EXCENV_EUNSUPPORTED; }
  const dim3 grid((unsigned)blocks), block(BLOCK);
  if (rc.V == VMAX) hipLaunchKernelGGL((rew_vjp_kernel<M, T, VMAX>), grid, block, 0, (hipStream_t)rc.stream, ka);
  else hipLaunchKernelGGL((rew_vjp_kernel<M, T, 1>), grid, block, 0, (hipStream_t)rc.stream, ka);
  g_last_launch = rew_vjp_name(rc.V);
  return check_launch("excenv_rew_vjp");
}

// EnvVTable::rew_vjp (launch.hpp), instantiated in rew_vjp.hip. The reward does not read the saturated model's tables: its entry is
// the linear PMSM's.
template <template <typename> class MT> int rew_vjp_entry(const RewVjpCall& rc) {
  if constexpr (MT<float>::HAS_LUT) return rew_vjp_entry<Pmsm>(rc);
  else return EXCENV_BY_DTYPE(launch_rew_vjp, MT, rc);
}

}  // namespace excenv
