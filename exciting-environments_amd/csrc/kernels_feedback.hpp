// Closed-loop trajectories: sim_feedback_kernel runs all N = K * substeps solver steps of a trajectory in one persistent launch like
// sim_ahead_kernel (kernels.hpp), but computes every action row itself from the observation row it has just saved — affine output
// feedback with optional integral action and a feedforward row:
//   acc = ff[k][q];  acc += z[q];  acc = fma(Gp[q][o], obs_n[o], acc) for o = 0 .. OW-1;  a[k][q] = clamp(acc, lo, hi)
//   zi = 0;  zi = fma(Gi[q][o], obs_n[o], zi) for o = 0 .. OW-1;  z[q] = clamp(z[q] + action_stepsize * zi, lo, hi)
// The loop is the one-environment-per-lane general form of sim_ahead_body.inc under EXCENV_SEM_STEP — load_ctx<true>, env_step,
// M::observe, the control columns — with the action in registers instead of memory, so a trajectory is bit for bit what the open-loop
// kernel returns for the applied actions. The gains are read once and stay in registers (A * OW values per gain set). Integral action,
// feedforward, actions_out and the state trajectory are launch-uniform run-time branches on NULL pointers. The saturated PMSM gathers
// from its tables in global memory. No LDS, no inline assembly, no scratch. Instantiated in feedback_<model>.hip only.
#pragma once
#include "feedback.hpp"
#include "launch.hpp"

namespace excenv {

template <typename T, class M> struct FeedbackArgs {
  KProps<T, M> kp;
  int64_t B, K;
  int32_t substeps;
  int32_t n_control;
  const T* state_in[M::S];
  T* last_state[M::S];
  T* obs;          // [N + 1][O + n_control][B]
  T* straj[M::S];  // [N + 1][B] each; straj[0] == nullptr: no state trajectory
  int32_t control_idx[EXCENV_MAX_CONTROL];
  const T* reference[EXCENV_MAX_CONTROL];
  const T* gain;       // [A][OW][Bg]
  const T* igain;      // [A][OW][Bg] or nullptr: no integral action
  int64_t g_se, g_sb;  // element strides of the gains: between entries (Bg) and between environments (Bg == B ? 1 : 0)
  const T* ff;         // [K][A][B] or nullptr
  const T* z_in;       // [A][B] or nullptr (zeros)
  T* z_out;            // [A][B]; written with integral action only
  T* actions_out;      // [K][A][B] or nullptr
  T clip_lo, clip_hi;  // both clamps: max_nan / min_nan (a NaN passes through); -inf / +inf change nothing
  T action_dt;         // obs_stepsize * substeps, folded in double on the host
  T dt, env_tau, adv_coef;
};

// Register caps as sim_min_waves gives them to the general trajectory kernel (kernels.hpp): the compiler's choice everywhere but for
// the pendulum in fp64, whose second wave per SIMD stays — and for acrobot Tsit5 in fp64, which the gain registers took to 258, two
// past the second wave. The counts are in DESIGN.md §4.11.
template <class M, typename T, int SOLVER> constexpr int feedback_min_waves() {
  if (M::ID == EXCENV_ACROBOT && sizeof(T) == 8 && SOLVER == EXCENV_TSIT5) return 2;
  return sim_min_waves<M, T, true, false, false, -2, SOLVER>();
}

template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(feedback_min_waves<M, T, SOLVER>())))
sim_feedback_kernel(const FeedbackArgs<T, M> ka) {
  constexpr int S = M::S, A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  Ctx<T, M> c;
  load_ctx<true>(c, ka.kp, (i < ka.B) ? i : 0, ka.dt, ka.env_tau, ka.adv_coef);  // lut_lds = 0: the tables stay in global memory
  c.lin_stop = T(0);  // the trajectory clock of EXCENV_SEM_AHEAD: not read by a step
  c.lin_div = T(1);
  c.lin_last = 0;
  if (i >= ka.B) return;

  T st[S];
#pragma unroll
  for (int j = 0; j < S; ++j) st[j] = ka.state_in[j][i];
  T memo[1][6];  // look-up model: the table values at the current operating point (sim_ahead_body.inc)
  if constexpr (M::HAS_LUT) M::lookup(st[3], st[4], c, memo[0]);

  // reference-tracking columns: constant along the trajectory, normalised once, exactly as the open-loop general kernel does
  T cref[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    cref[j] = T(0);
    if (j < ka.n_control) {
      const int f = ka.control_idx[j];
      T lo = c.smin[0], hi = c.smax[0];
#pragma unroll
      for (int q = 1; q < S; ++q) {
        lo = (f == q) ? c.smin[q] : lo;
        hi = (f == q) ? c.smax[q] : hi;
      }
      cref[j] = normalize(ka.reference[j][i], lo, hi);
    }
  }

  // the gains of this lane's environment, for the whole trajectory (columns past O + n_control: never read)
  const int OW = O + ka.n_control;
  const bool integral = ka.igain != nullptr;
  T gp[A][O + NC], gi[A][O + NC], z[A];
  {
    const T* g = ka.gain + i * ka.g_sb;
    const T* h = integral ? ka.igain + i * ka.g_sb : g;
#pragma unroll
    for (int q = 0; q < A; ++q) {
#pragma unroll
      for (int o = 0; o < O + NC; ++o) {
        gp[q][o] = gi[q][o] = T(0);
        if (o < OW) {
          gp[q][o] = g[(q * OW + o) * ka.g_se];
          if (integral) gi[q][o] = h[(q * OW + o) * ka.g_se];
        }
      }
      z[q] = (integral && ka.z_in != nullptr) ? ka.z_in[q * ka.B + i] : T(0);
    }
  }

  const int64_t N = ka.K * ka.substeps;
  const bool with_states = ka.straj[0] != nullptr;
  const int64_t o_row = (int64_t)OW * ka.B;
  T* orow = ka.obs + i;
  int64_t s_off = i;

  // the feedforward row of action k, and the next one in flight
  const bool with_ff = ka.ff != nullptr && ka.K > 0;
  const int64_t klast = ka.K - 1;
  T ffc[A], ffn[A];
#pragma unroll
  for (int q = 0; q < A; ++q) ffc[q] = ffn[q] = with_ff ? ka.ff[q * ka.B + i] : T(0);

  T a[A];
#pragma unroll
  for (int q = 0; q < A; ++q) a[q] = T(0);
  int64_t k = 0;
  int32_t sub = 0;
  for (int64_t n = 0;; ++n) {
    const bool act = sub == 0 && n < N;  // row n is an action row (wave-uniform)
    // row k + 1 of the feedforward is requested before row n is saved and step n is computed, and first read one action later; the
    // index is clamped, so the load is unconditional (DESIGN.md §4.1 "Pipeline")
    if (act && with_ff) {
      const int64_t k1 = (k < klast) ? k + 1 : klast;
#pragma unroll
      for (int q = 0; q < A; ++q) ffn[q] = ka.ff[(k1 * A + q) * ka.B + i];
    }
    // ---- save row n
    T ob[O];
    M::observe(st, c, ob);
#pragma unroll
    for (int q = 0; q < O; ++q) {
      const T tmp[1] = {ob[q]};
      store_stream<T, 1>(orow + q * ka.B, tmp);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      if (j < ka.n_control) {
        const T tmp[1] = {cref[j]};
        store_v<T, 1>(orow + (O + j) * ka.B, tmp);
      }
    }
    if (with_states) {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const T tmp[1] = {st[j]};
        store_stream<T, 1>(ka.straj[j] + s_off, tmp);
      }
    }
    orow += o_row;
    s_off += ka.B;
    if (n == N) break;
    // ---- the policy on the row just saved
    if (act) {
#pragma unroll
      for (int q = 0; q < A; ++q) {
        T acc = ffc[q];
        if (integral) acc = acc + z[q];
#pragma unroll
        for (int o = 0; o < O; ++o) acc = xfma(gp[q][o], ob[o], acc);
#pragma unroll
        for (int j = 0; j < NC; ++j)
          if (j < ka.n_control) acc = xfma(gp[q][O + j], cref[j], acc);
        a[q] = min_nan(max_nan(acc, ka.clip_lo), ka.clip_hi);
        if (integral) {
          T zi = T(0);
#pragma unroll
          for (int o = 0; o < O; ++o) zi = xfma(gi[q][o], ob[o], zi);
#pragma unroll
          for (int j = 0; j < NC; ++j)
            if (j < ka.n_control) zi = xfma(gi[q][O + j], cref[j], zi);
          z[q] = min_nan(max_nan(z[q] + ka.action_dt * zi, ka.clip_lo), ka.clip_hi);
        }
        ffc[q] = ffn[q];
      }
      if (ka.actions_out != nullptr) {
#pragma unroll
        for (int q = 0; q < A; ++q) {
          const T tmp[1] = {a[q]};
          store_stream<T, 1>(ka.actions_out + (k * A + q) * ka.B + i, tmp);
        }
      }
    }
    // ---- step n under the held action
    env_step<M, SOLVER>(st, a, c, M::HAS_LUT ? &memo[0] : nullptr);
    if (++sub == ka.substeps) {
      sub = 0;
      ++k;
    }
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const T tmp[1] = {st[j]};
    store_v<T, 1>(ka.last_state[j] + i, tmp);
  }
  if (integral) {
#pragma unroll
    for (int q = 0; q < A; ++q) ka.z_out[q * ka.B + i] = z[q];
  }
}

// Packs FeedbackArgs and launches the instantiation of the call's solver
template <class M, typename T> static int launch_feedback(const FeedbackCall& fc) {
  FeedbackArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, fc.props);
  double coef;
  if (int rc = pmsm_coef<M>(fc.props, fc.env_tau, &coef)) return rc;
  ka.B = fc.B;
  ka.K = fc.K;
  ka.substeps = fc.substeps;
  ka.n_control = fc.control ? fc.control->n_control : 0;
  for (int j = 0; j < M::S; ++j) {
    if (!fc.state_in[j] || !fc.last_state[j]) { set_error("excenv_sim_feedback: state pointer %d is NULL", j); return EXCENV_ENULL; }
    if (fc.state_traj && !fc.state_traj[j]) { set_error("excenv_sim_feedback: state_traj pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.state_in[j] = (const T*)fc.state_in[j];
    ka.last_state[j] = (T*)fc.last_state[j];
    ka.straj[j] = fc.state_traj ? (T*)fc.state_traj[j] : nullptr;
  }
  ka.obs = (T*)fc.obs_traj;
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = fc.control->control_idx[j];
    ka.reference[j] = (const T*)fc.control->reference[j];
  }
  const excenv_feedback_t& p = *fc.policy;
  ka.gain = (const T*)p.gain;
  ka.igain = (const T*)p.integral_gain;
  ka.g_se = p.gain_batch;
  ka.g_sb = (p.gain_batch == fc.B && fc.B > 1) ? 1 : 0;
  ka.ff = (const T*)p.feedforward;
  ka.z_in = (const T*)p.z_in;
  ka.z_out = (T*)p.z_out;
  ka.actions_out = (T*)fc.actions_out;
  ka.clip_lo = (T)p.clip_lo;
  ka.clip_hi = (T)p.clip_hi;
  ka.action_dt = (T)(fc.obs_stepsize * (double)fc.substeps);
  ka.dt = (T)fc.obs_stepsize;
  ka.env_tau = (T)fc.env_tau;
  ka.adv_coef = (T)coef;
  if (fc.B == 0) return EXCENV_OK;
  const int64_t blocks = (fc.B + BLOCK - 1) / BLOCK;
  if (blocks > (int64_t)0x7fffffff) {
    set_error("excenv_sim_feedback: ceil(B / %d) = %lld workgroups exceed one launch", BLOCK, (long long)blocks);
    return EXCENV_EINVAL;
  }
  const dim3 grid((unsigned)blocks), block(BLOCK);
  const hipStream_t stream = (hipStream_t)fc.stream;
  with_solver(fc.solver, [&](auto solver) {  // (check_common has validated the id)
    hipLaunchKernelGGL((sim_feedback_kernel<M, T, decltype(solver)::value>), grid, block, 0, stream, ka);
    return true;
  });
  g_last_launch = feedback_name();
  return check_launch("excenv_sim_feedback");
}

// EnvVTable::sim_feedback (launch.hpp): a model's translation unit feedback_<model>.hip instantiates it
template <template <typename> class MT> int feedback_entry(const FeedbackCall& fc) { return EXCENV_BY_DTYPE(launch_feedback, MT, fc); }

}  // namespace excenv
