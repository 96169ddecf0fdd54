// Reverse mode of the closed-loop trajectory kernel (kernels_feedback.hpp): one excenv_sim_feedback_vjp call is
//   feedback_z_rows_kernel     the integrator rows z_1 .. z_K again, by the forward's own recurrence over the saved observation rows
//                              (with integral action only: the forward does not store them, the reverse pass needs their clamp masks)
//   sim_feedback_vjp_kernel    one persistent launch, rows N down to 0: the row pipeline of sim_ahead_vjp_kernel (kernels_vjp.hpp) under
//                              EXCENV_SEM_STEP, one environment per lane, with the transposed policy at every action row. It carries the
//                              integrator's cotangent next to the state's and writes grad_ff / grad_zi rows, grad_state0 and grad_z0.
//   feedback_gain_grad_kernel  grad_G[q][o] = sum_k row_k[q] * ob_k[o] per environment, from the rows just written and the stored
//                              observation rows: A * OW accumulators that stay out of the reverse kernel; one launch, both gain sets
//   (gain_batch == 1)          the deterministic batch sum of param_sum.hip, EXCENV_MAX_STATIC entries per call
// The step's arithmetic is env_step_vjp<M, SOLVER, /*AHEAD=*/false> and M::observe_vjp, exactly as step_vjp_kernel uses them. The
// read-only gains the reverse kernel needs (the O observation columns of both sets: obb of the contract) live in LDS in every
// instantiation: one copy per workgroup for a broadcast gain set (every lane reads the same address), a private odd-stride run per lane
// for per-environment gains — no instantiation's register count depends on A * O. No inline assembly, no scratch, no atomics.
// Instantiated in feedback_vjp_<model>.hip only.
#pragma once
#include "feedback_vjp.hpp"
#include "kernels_vjp.hpp"

namespace excenv {

int launch_param_sum(int dtype, int64_t B, int n, const void* const* per_env, void* out, void* workspace, hipStream_t stream);  // param_sum.hip

template <typename T, class M> struct FeedbackVjpArgs {
  KProps<T, M> kp;
  int64_t B, K;
  int32_t substeps, n_control;
  const T* obs;            // [N + 1][OW][B]: the pre-pass and the gain kernel read it
  const T* actions;        // [K][A][B]: the applied actions
  const T* straj[M::S];    // [N + 1][B]
  const T* z_in;           // [A][B] or nullptr (zeros): the pre-pass starts from it
  T* zrows;                // [K][A][B]: row k holds z_{k+1}; nullptr without integral action
  const T* gain;           // [A][OW][Bg]
  const T* igain;          // [A][OW][Bg] or nullptr: no integral action
  int64_t g_se, g_sb;      // element strides of the gains: between entries (Bg) and between environments (Bg == B ? 1 : 0)
  int32_t gains_per_env;   // the LDS form: a private run per lane (1) or one copy per workgroup (0)
  const T* g_obs;          // [N + 1][OW][B] or nullptr
  const T* g_straj[M::S];  // [N + 1][B] or nullptr, per leaf
  const T* g_last[M::S];   // [B] or nullptr, per leaf
  const T* g_actions;      // [K][A][B] or nullptr
  const T* g_z;            // [A][B] or nullptr
  T* g_state0[M::S];       // [B]
  T* g_ff;                 // [K][A][B]
  T* g_zi;                 // [K][A][B], with integral action
  T* g_z0;                 // [A][B], with integral action
  T clip_lo, clip_hi;
  T action_dt;             // obs_stepsize * substeps, folded in double on the host like the forward's
  T dt, env_tau, adv_coef;
};

// The lane's run of gains in LDS: both sets' O observation columns, padded to an odd number of elements (the 32 lanes of a
// ds_read_b64 group hit distinct banks, as vjp_pgrad_in_lds's accumulators do)
template <class M> constexpr int feedback_vjp_gain_stride() { return (2 * M::A * M::O) | 1; }
template <class M, typename T> constexpr size_t feedback_vjp_lds_bytes(bool per_env) {
  return sizeof(T) * (size_t)feedback_vjp_gain_stride<M>() * (per_env ? BLOCK : 1);
}

// z_1 .. z_K into zrows[K][A][B], one environment per lane: the forward's statements (kernels_feedback.hpp) on the stored observation
// row of every action row — the stored columns are the registers the forward multiplied, references included
template <class M, typename T> __global__ void __launch_bounds__(BLOCK) feedback_z_rows_kernel(const FeedbackVjpArgs<T, M> ka) {
  constexpr int A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= ka.B) return;
  const int OW = O + ka.n_control;
  T gi[A][O + NC], z[A];
  {
    const T* h = ka.igain + i * ka.g_sb;
#pragma unroll
    for (int q = 0; q < A; ++q) {
#pragma unroll
      for (int o = 0; o < O + NC; ++o) gi[q][o] = (o < OW) ? h[(q * OW + o) * ka.g_se] : T(0);
      z[q] = (ka.z_in != nullptr) ? ka.z_in[q * ka.B + i] : T(0);
    }
  }
  const int64_t o_row = (int64_t)OW * ka.B * ka.substeps;  // from one action row's observation row to the next one's
  const T* orow = ka.obs + i;
  for (int64_t k = 0; k < ka.K; ++k) {
    T ob[O + NC];
#pragma unroll
    for (int o = 0; o < O + NC; ++o) ob[o] = (o < OW) ? orow[o * ka.B] : T(0);
#pragma unroll
    for (int q = 0; q < A; ++q) {
      T zi = T(0);
#pragma unroll
      for (int o = 0; o < O; ++o) zi = xfma(gi[q][o], ob[o], zi);
#pragma unroll
      for (int j = 0; j < NC; ++j)
        if (j < ka.n_control) zi = xfma(gi[q][O + j], ob[O + j], zi);
      z[q] = min_nan(max_nan(z[q] + ka.action_dt * zi, ka.clip_lo), ka.clip_hi);
      ka.zrows[(k * A + q) * ka.B + i] = z[q];
    }
    orow += o_row;
  }
}

// grad_G[q][o][i] = sum over k (ascending) of rows[k][q][i] * obs[k * substeps][o][i], all OW columns; out is [A][OW][B]. blockIdx.y
// selects the gain set (its rows and its output): both sets' sums run side by side in one launch.
template <typename T> struct FeedbackGainGradSets {
  const T* rows[2];
  T* out[2];
};
template <class M, typename T>
__global__ void __launch_bounds__(BLOCK) feedback_gain_grad_kernel(const FeedbackGainGradSets<T> sets, const T* __restrict__ obs, int64_t B, int64_t K,
                                                                 int32_t substeps, int32_t n_control) {
  constexpr int A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= B) return;
  const T* __restrict__ rows = sets.rows[blockIdx.y];
  T* __restrict__ out = sets.out[blockIdx.y];
  const int OW = O + n_control;
  T acc[A][O + NC];
#pragma unroll
  for (int q = 0; q < A; ++q)
#pragma unroll
    for (int o = 0; o < O + NC; ++o) acc[q][o] = T(0);
  const int64_t o_row = (int64_t)OW * B * substeps;
  const T* orow = obs + i;
  for (int64_t k = 0; k < K; ++k) {
    T ob[O + NC], r[A];
#pragma unroll
    for (int o = 0; o < O + NC; ++o) ob[o] = (o < OW) ? orow[o * B] : T(0);
#pragma unroll
    for (int q = 0; q < A; ++q) r[q] = rows[(k * A + q) * B + i];
#pragma unroll
    for (int q = 0; q < A; ++q)
#pragma unroll
      for (int o = 0; o < O + NC; ++o) acc[q][o] = acc[q][o] + r[q] * ob[o];
    orow += o_row;
  }
#pragma unroll
  for (int q = 0; q < A; ++q)
#pragma unroll
    for (int o = 0; o < O + NC; ++o)
      if (o < OW) out[(q * OW + o) * B + i] = acc[q][o];
}

// One lane owns one environment for the whole trajectory. Per solver step it reads one saved state row and the cotangent rows that
// are present (launch-uniform NULL branches: an absent group loads nothing); per action row also the applied action, the integrator
// row and the grad_actions row, and writes one grad_ff (and grad_zi) row. The next iteration's rows are requested before the step's
// arithmetic, index clamped so that the loads are unconditional (DESIGN.md §4.1 "Pipeline") — behind it in the instantiations that
// vjp_late_cotangents names, whose registers are needed during the step.
template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) sim_feedback_vjp_kernel(const FeedbackVjpArgs<T, M> ka) {
  constexpr int S = M::S, A = M::A, O = M::O;
  constexpr bool LEAN = vjp_lean_trig<T>();
  static_assert(!M::HAS_LUT, "no reverse mode for the saturated PMSM");
  constexpr int GSTRIDE = feedback_vjp_gain_stride<M>();
  extern __shared__ __attribute__((aligned(16))) unsigned char feedback_vjp_lds[];
  T* const glds = reinterpret_cast<T*>(feedback_vjp_lds);
  const int64_t blk0 = (int64_t)blockIdx.x * BLOCK;  // first environment of the workgroup
  const unsigned lane0 = threadIdx.x;
  unsigned lane = lane0;  // refreshed per row, as in sim_ahead_vjp_kernel: (uniform pointer + uniform offset) + one 32-bit lane offset
  const int64_t i0 = blk0 + lane0;
  const int64_t B = ka.B;
  const int32_t K = (int32_t)ka.K, N = K * ka.substeps;  // (host: N fits; 32-bit row counters: scalar registers are this kernel's scarce ones)
  const int64_t OW = O + ka.n_control;
  const bool integral = ka.igain != nullptr;
  Ctx<T, M> c;
  load_ctx<false>(c, ka.kp, 0, ka.dt, ka.env_tau, ka.adv_coef);
  c.lin_stop = T(0);  // the trajectory clock of EXCENV_SEM_AHEAD: not read by a step
  c.lin_div = T(1);
  c.lin_last = 0;
  // the refined reciprocals go to scalar registers where vector registers are the scarce ones (vjp_uniform): the four-leaf models
  // and PMSM. The small models have vector registers to spare and, with this kernel's streams, no scalar ones: there the move made
  // the allocator reserve scratch for a scalar spill (pendulum Tsit5 in fp64).
  if constexpr (M::S >= 4 || M::IS_PMSM) {
#pragma unroll
    for (int j = 0; j < S; ++j) c.nrm[j].y = vjp_uniform(c.nrm[j].y);
#pragma unroll
    for (int j = 0; j < (M::ND > 0 ? M::ND : 1); ++j) c.den[j].y = vjp_uniform(c.den[j].y);
  }

  // the gains' observation columns into LDS: entry (set, q, o) at (set * A + q) * O + o of the lane's run (set 0: Gp, 1: Gi)
  const T* gl = glds;
  if (ka.gains_per_env) {
    T* mine = glds + threadIdx.x * GSTRIDE;
    if (i0 < B) {
#pragma unroll
      for (int q = 0; q < A; ++q)
#pragma unroll
        for (int o = 0; o < O; ++o) {
          mine[q * O + o] = ka.gain[(q * OW + o) * ka.g_se + i0 * ka.g_sb];
          mine[(A + q) * O + o] = integral ? ka.igain[(q * OW + o) * ka.g_se + i0 * ka.g_sb] : T(0);
        }
    }
    gl = mine;
  } else {
    for (int e = threadIdx.x; e < A * O; e += BLOCK) {
      const int q = e / O, o = e % O;
      glds[e] = ka.gain[(q * OW + o) * ka.g_se];
      glds[A * O + e] = integral ? ka.igain[(q * OW + o) * ka.g_se] : T(0);
    }
    __syncthreads();
  }
  if (i0 >= B) return;

  auto load_state_row = [&](int64_t n, T (&sv)[S]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j) sv[j] = ((ka.straj[j] + (n * B + blk0)) + lane)[0];
  };
  auto load_gobs_row = [&](int64_t n, T (&go)[O]) __attribute__((always_inline)) {
    if (ka.g_obs != nullptr) {
#pragma unroll
      for (int q = 0; q < O; ++q) go[q] = ((ka.g_obs + ((n * OW + q) * B + blk0)) + lane)[0];
    }
  };
  auto load_gst_row = [&](int64_t n, T (&gs)[S]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j)
      if (ka.g_straj[j] != nullptr) gs[j] = ((ka.g_straj[j] + (n * B + blk0)) + lane)[0];
  };
  auto load_krow = [&](const T* base, int64_t k, T (&a)[A]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < A; ++q) a[q] = ((base + ((k * A + q) * B + blk0)) + lane)[0];
  };
  auto store_krow = [&](T* base, int64_t k, const T (&a)[A]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < A; ++q) {
      const T tmp[1] = {a[q]};
      store_stream<T, 1>((base + ((k * A + q) * B + blk0)) + lane, tmp);
    }
  };

  T sb[S], zb[A], ab[A];  // cotangents of the carried state, of z_{k+1} and of the held action
  T om_c = T(0);  // PMSM: omega_el is a constant of the trajectory — row 0's value stands for every row's (same bits)
  if constexpr (M::IS_PMSM) om_c = ((ka.straj[6] + blk0) + lane)[0];
#pragma unroll
  for (int q = 0; q < A; ++q) {
    ab[q] = T(0);
    zb[q] = (integral && ka.g_z != nullptr) ? ((ka.g_z + (q * B + blk0)) + lane)[0] : T(0);
  }
  // cotangent of a saved row -> cotangent of the carried state
  auto consume = [&](const T (&sv)[S], const T (&go)[O], const T (&gs)[S]) __attribute__((always_inline)) {
    T r[S];
#pragma unroll
    for (int j = 0; j < S; ++j) r[j] = T(0);
    if (ka.g_obs != nullptr) M::template observe_vjp<LEAN>(sv, c, go, r);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (ka.g_straj[j] != nullptr) r[j] = r[j] + gs[j];
      sb[j] = sb[j] + r[j];
    }
  };

  T svh[S], svc[S], svn[S];  // saved rows n, n - 1 and (in flight) n - 2
  T go[O], gs[S];            // cotangent rows of row n
  T ac[A], an[A];            // action row k of step n - 1, and of step n - 2 (in flight)
  load_state_row(N, svh);
#pragma unroll
  for (int j = 0; j < S; ++j) sb[j] = (ka.g_last[j] != nullptr) ? ((ka.g_last[j] + blk0) + lane)[0] : T(0);  // last_state is row N
  load_gobs_row(N, go);
  load_gst_row(N, gs);
  load_state_row(N > 0 ? N - 1 : 0, svc);
  if (N > 0) load_krow(ka.actions, K - 1, ac);

  const int32_t sub_last = ka.substeps - 1;
  int32_t k = K - 1;  // (k, sub): action row and sub-step of step n - 1
  int32_t sub = sub_last;
  for (int32_t n = N;; --n) {
    lane = (unsigned)__builtin_amdgcn_mov_dpp((int)lane0, 0xE4, 0xF, 0xF, false);  // (not a loop invariant to the optimiser)
    consume(svh, go, gs);
    if (n == 0) break;
    // step n - 1 leads from row n - 1 to row n; what the next iteration reads is requested now
    int32_t kp = k;
    int32_t subp = sub - 1;
    if (subp < 0) {
      subp = sub_last;
      kp = (k > 0) ? k - 1 : 0;
    }
    const bool act = sub == 0;  // row n - 1 is the action row of k (wave-uniform): the policy is transposed behind this step
    constexpr bool LATE = vjp_late_cotangents<M, T, SOLVER, 1>();
    constexpr bool LATE_ROW = LATE && M::IS_PMSM && sizeof(T) == 8;
    T zr[A], ga[A];  // z_{k+1} and the grad_actions row of k
#pragma unroll
    for (int q = 0; q < A; ++q) zr[q] = ga[q] = T(0);
    auto load_policy_rows = [&]() __attribute__((always_inline)) {
      if (act) {
        if (integral) load_krow(ka.zrows, k, zr);
        if (ka.g_actions != nullptr) load_krow(ka.g_actions, k, ga);
      }
    };
    if constexpr (!LATE) {
      load_gobs_row(n - 1, go);
      load_gst_row(n - 1, gs);
      load_policy_rows();
    }
    if constexpr (!LATE_ROW) {
      load_state_row(n > 1 ? n - 2 : 0, svn);
      load_krow(ka.actions, kp, an);
    }
    T s0[S], s1[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      s0[j] = svc[j];
      s1[j] = svh[j];
    }
    if constexpr (M::IS_PMSM) s0[6] = s1[6] = om_c;
    {
      T geps0 = T(0), g0[A], g1[A];
      env_step_vjp<M, SOLVER, false>(s0, s1, ac, ac, 0, 0, c, T(0), sb, geps0, g0, g1);
#pragma unroll
      for (int q = 0; q < A; ++q) ab[q] = ab[q] + ((SOLVER == EXCENV_EULER) ? g0[q] : g0[q] + g1[q]);  // the c_i == 1 stages read the same row
    }
    if constexpr (LATE_ROW) {
      load_state_row(n > 1 ? n - 2 : 0, svn);
      load_krow(ka.actions, kp, an);
    }
    if constexpr (LATE) {
      load_gobs_row(n - 1, go);
      load_gst_row(n - 1, gs);
      load_policy_rows();
    }
    if (act) {
      // the transposed policy at row n - 1: clamps have derivative 0 on and outside their bounds, a NaN compares false
      T pre[A], gzi[A], obb[O];
#pragma unroll
      for (int o = 0; o < O; ++o) obb[o] = T(0);
#pragma unroll
      for (int q = 0; q < A; ++q) {
        const T abq = ab[q] + ga[q];
        pre[q] = (ac[q] > ka.clip_lo && ac[q] < ka.clip_hi) ? abq : T(0);
        ab[q] = T(0);
      }
      store_krow(ka.g_ff, k, pre);
#pragma unroll
      for (int q = 0; q < A; ++q)
#pragma unroll
        for (int o = 0; o < O; ++o) obb[o] = obb[o] + gl[q * O + o] * pre[q];
      if (integral) {
#pragma unroll
        for (int q = 0; q < A; ++q) {
          const T zpre = (zr[q] > ka.clip_lo && zr[q] < ka.clip_hi) ? zb[q] : T(0);
          gzi[q] = ka.action_dt * zpre;
          zb[q] = pre[q] + zpre;
        }
        store_krow(ka.g_zi, k, gzi);
#pragma unroll
        for (int q = 0; q < A; ++q)
#pragma unroll
          for (int o = 0; o < O; ++o) obb[o] = obb[o] + gl[(A + q) * O + o] * gzi[q];
      }
      M::template observe_vjp<LEAN>(s0, c, obb, sb);
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      svh[j] = svc[j];
      svc[j] = svn[j];
    }
#pragma unroll
    for (int q = 0; q < A; ++q) ac[q] = an[q];
    k = kp;
    sub = subp;
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const T tmp[1] = {sb[j]};
    store_v<T, 1>((ka.g_state0[j] + blk0) + lane, tmp);
  }
  if (integral) {
#pragma unroll
    for (int q = 0; q < A; ++q) ((ka.g_z0 + (q * B + blk0)) + lane)[0] = zb[q];
  }
}

// Packs FeedbackVjpArgs and enqueues the launches of one call (the header of this file) on the call's stream
template <class M, typename T> static int launch_feedback_vjp(const FeedbackVjpCall& fc) {
  constexpr int A = M::A, O = M::O;
  const char* fn = "excenv_sim_feedback_vjp";
  FeedbackVjpArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  if (int rc = reverse_preamble(fn, ka, fc.props, fc.obs_stepsize, fc.env_tau, false)) return rc;
  const excenv_feedback_vjp_t& r = *fc.r;
  const bool integral = r.integral_gain != nullptr;
  ka.B = fc.B;
  ka.K = fc.K;
  ka.substeps = fc.substeps;
  ka.n_control = fc.control ? fc.control->n_control : 0;
  const int OW = O + ka.n_control;
  for (int j = 0; j < M::S; ++j) {
    if (!r.state_traj[j] || !r.grad_state0[j]) { set_error("%s: state pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    ka.straj[j] = (const T*)r.state_traj[j];
    ka.g_straj[j] = r.grad_states ? (const T*)r.grad_states[j] : nullptr;
    ka.g_last[j] = r.grad_last_state ? (const T*)r.grad_last_state[j] : nullptr;
    ka.g_state0[j] = (T*)r.grad_state0[j];
  }
  ka.obs = (const T*)r.obs_traj;
  ka.actions = (const T*)r.actions;
  ka.z_in = (const T*)r.z_in;
  ka.gain = (const T*)r.gain;
  ka.igain = (const T*)r.integral_gain;
  ka.g_se = r.gain_batch;
  ka.g_sb = (r.gain_batch == fc.B && fc.B > 1) ? 1 : 0;
  ka.gains_per_env = (int32_t)ka.g_sb;
  ka.g_obs = (const T*)r.grad_obs;
  ka.g_actions = (const T*)r.grad_actions;
  ka.g_z = (const T*)r.grad_z;
  ka.g_ff = (T*)r.grad_ff;
  ka.g_zi = (T*)r.grad_zi;
  ka.g_z0 = (T*)r.grad_z0;
  ka.clip_lo = (T)r.clip_lo;
  ka.clip_hi = (T)r.clip_hi;
  ka.action_dt = (T)(fc.obs_stepsize * (double)fc.substeps);
  if (fc.B == 0) return EXCENV_OK;
  if (fc.K > (int64_t)0x7fffffff / fc.substeps) {
    set_error("%s: K * substeps = %lld * %d rows exceed one launch", fn, (long long)fc.K, (int)fc.substeps);
    return EXCENV_EINVAL;
  }
  const int64_t blocks = (fc.B + BLOCK - 1) / BLOCK;
  if (blocks > (int64_t)0x7fffffff) {
    set_error("%s: ceil(B / %d) = %lld workgroups exceed one launch", fn, BLOCK, (long long)blocks);
    return EXCENV_EINVAL;
  }
  // the workspace (feedback_vjp.hpp): z rows, the per-environment terms of a broadcast gain set, the batch sum's partials
  char* ws = (char*)fc.workspace;
  ka.zrows = integral ? (T*)ws : nullptr;
  ws += feedback_vjp_z_bytes(A, (int)sizeof(T), fc.B, fc.K, integral);
  T* terms = (T*)ws;
  ws += feedback_vjp_terms_bytes(A, OW, (int)sizeof(T), fc.B, r.gain_batch, integral);
  void* partials = ws;
  const dim3 grid((unsigned)blocks), block(BLOCK);
  const hipStream_t stream = (hipStream_t)fc.stream;
  if (integral && fc.K > 0) {
    hipLaunchKernelGGL((feedback_z_rows_kernel<M, T>), grid, block, 0, stream, ka);
    if (int rc = check_launch("excenv_sim_feedback_vjp (integrator rows)")) return rc;
  }
  const size_t lds = ka.gains_per_env ? feedback_vjp_lds_bytes<M, T>(true) : feedback_vjp_lds_bytes<M, T>(false);
  with_solver(fc.solver, [&](auto solver) {  // (check_common has validated the id)
    launch_dyn(sim_feedback_vjp_kernel<M, T, decltype(solver)::value>, grid, block, lds, stream, ka);
    return true;
  });
  g_last_launch = feedback_vjp_name();
  if (int rc = check_launch(fn)) return rc;
  // the gain gradients from the rows just written: per environment (one launch for the sets that are wanted), then (one gain set for
  // all) summed over the batch
  const bool summed = r.gain_batch == 1;
  const int n_entries = A * OW;
  const T* rows[2] = {ka.g_ff, ka.g_zi};
  T* outs[2] = {(T*)r.grad_gain, (T*)r.grad_integral_gain};
  FeedbackGainGradSets<T> sets{};
  T* per_env[2] = {nullptr, nullptr};
  unsigned n_sets = 0;
  for (int set = 0; set < 2; ++set) {
    if (!outs[set]) continue;
    per_env[set] = summed ? terms + (int64_t)set * n_entries * fc.B : outs[set];
    sets.rows[n_sets] = rows[set];
    sets.out[n_sets++] = per_env[set];
  }
  if (n_sets > 0) {
    hipLaunchKernelGGL((feedback_gain_grad_kernel<M, T>), dim3((unsigned)blocks, n_sets), block, 0, stream, sets, ka.obs, fc.B, fc.K, fc.substeps,
                       ka.n_control);
    if (int rc = check_launch("excenv_sim_feedback_vjp (gain gradients)")) return rc;
  }
  for (int set = 0; summed && set < 2; ++set) {
    if (!outs[set]) continue;
    for (int e0 = 0; e0 < n_entries; e0 += EXCENV_MAX_STATIC) {
      const int n = (n_entries - e0 < EXCENV_MAX_STATIC) ? n_entries - e0 : EXCENV_MAX_STATIC;
      const void* leaves[EXCENV_MAX_STATIC];
      for (int j = 0; j < n; ++j) leaves[j] = per_env[set] + (int64_t)(e0 + j) * fc.B;
      if (launch_param_sum(fc.dtype, fc.B, n, leaves, outs[set] + e0, partials, stream) != EXCENV_OK) {
        set_error("%s: HIP launch failed (batch sum of the gain gradients)", fn);
        return EXCENV_EHIP;
      }
    }
  }
  return EXCENV_OK;
}

// EnvVTable::sim_feedback_vjp (launch.hpp): a model's translation unit feedback_vjp_<model>.hip instantiates it
template <template <typename> class MT> int feedback_vjp_entry(const FeedbackVjpCall& fc) {
  if constexpr (MT<float>::HAS_LUT) {
    set_error("excenv_sim_feedback_vjp: the saturated PMSM (pmsm_lut) has no reverse mode");
    return EXCENV_EUNSUPPORTED;
  } else {
    return EXCENV_BY_DTYPE(launch_feedback_vjp, MT, fc);
  }
}

}  // namespace excenv
