// Reverse mode of the policy rollout (kernels_policy.hpp; DESIGN.md §4.15, include/excenv.h excenv_policy_vjp_t): one
// excenv_sim_policy_vjp call is one persistent launch of sim_policy_vjp_kernel, rows N down to 0. It is sim_feedback_vjp_kernel
// (kernels_feedback_vjp.hpp: the row pipeline of sim_ahead_vjp_kernel under EXCENV_SEM_STEP, one environment per lane, the step's
// arithmetic env_step_vjp<M, SOLVER, false> and M::observe_vjp) with the transposed multi-layer perceptron in place of the transposed
// gain block. It carries the state cotangent back through the dynamics and through the network with respect to the network's INPUT
// only, and writes grad_raw[k], the cotangent of the pre-clamp output of every action row: no cross-lane reduction, no parameter
// gradient (that is a contraction over B * K independent samples, which the caller does on the rows the forward saved).
//   At an action row the lane evaluates the forward's statements again on the stored observation row and keeps EVERY hidden layer in
// its own LDS column h[l][j][lane] (the forward ping-pongs two buffers; the backward needs them all). The transposed layer l then
// reads d^l from that column and overwrites x^{l-1} with d^{l-1} in place once act' is taken, so the cotangents need no second
// buffer. A lane only reads what it wrote itself: no barrier. The weights are the forward's `const T* __restrict__` argument, read
// through wave-uniform indices (scalar loads, scalar operands of the FMAs). The transposed layer mirrors the forward's blocking: a
// block of UNR consecutive inputs as register accumulators, the loop over the layer's outputs j, W_l[j][i0 ..] one contiguous run.
//   One wavefront per workgroup (POLICY_BLOCK), two waves per SIMD by the register cap of the reverse kernels. No inline assembly, no
// scratch, no atomics. Instantiated in policy_vjp_<model>.hip only.
#pragma once
#include "kernels_policy.hpp"
#include "kernels_vjp.hpp"

namespace excenv {

template <typename T, class M> struct PolicyVjpArgs {
  KProps<T, M> kp;
  int64_t B, K;
  int32_t substeps, n_control;
  const T* obs;            // [N + 1][OW][B]: the rows of the action rows are read, all OW columns
  const T* actions;        // [K][A][B]: the applied actions
  const T* straj[M::S];    // [N + 1][B]
  const uint8_t* reset;    // [K][B] or nullptr (substeps == 1): step n was a reset
  int32_t n_layers, activation;
  int32_t widths[EXCENV_POLICY_MAX_LAYERS + 1];
  const T* g_obs;          // [N + 1][OW][B] or nullptr
  const T* g_straj[M::S];  // [N + 1][B] or nullptr, per leaf
  const T* g_last[M::S];   // [B] or nullptr, per leaf
  const T* g_actions;      // [K][A][B] or nullptr
  T* g_state0[M::S];       // [B]
  T* g_raw;                // [K][A][B]
  T clip_lo, clip_hi;
  T dt, env_tau, adv_coef;
};

// act'(h) times xb from the activation's VALUE h: ReLU passes xb where h > 0 (a NaN gets 0: torch's convention), tanh multiplies by
// 1 - h * h (two roundings: no contraction in this library)
template <typename T> __device__ __forceinline__ T policy_act_vjp(T xb, T h, int activation) {
  if (activation == EXCENV_ACT_TANH) return xb * (T(1) - h * h);
  return (h > T(0)) ? xb : T(0);
}

// Two waves per SIMD (256 registers per lane), the cap of every reverse kernel here — except in the instantiations that
// vjp_late_cotangents names (the fp64 RK adjoints of the four-leaf models and PMSM, which sim_ahead_vjp_kernel already fits into 256
// registers with one to spare): next to the step they hold this kernel's row pipeline AND the network's operands, and three of them
// (PMSM RK4 / Tsit5, acrobot Tsit5) reserved scratch at 256. They run at one wave per SIMD, where the second half of the register
// file takes what does not fit. With one wavefront per workgroup and the LDS of a wide fp64 network (96 KB) a CU holds one workgroup
// of those anyway.
template <class M, typename T, int SOLVER> constexpr int policy_vjp_min_waves() { return vjp_late_cotangents<M, T, SOLVER, 1>() ? 1 : 2; }

template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(POLICY_BLOCK) __attribute__((amdgpu_waves_per_eu(policy_vjp_min_waves<M, T, SOLVER>())))
sim_policy_vjp_kernel(const PolicyVjpArgs<T, M> ka, const T* __restrict__ params) {
  constexpr int S = M::S, A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL, BLK = POLICY_BLOCK, JB = POLICY_JB;
  constexpr int UNR = 32 / (int)sizeof(T);  // inputs per block of the transposed layer: 8 (fp32) or 4 (fp64) consecutive weights of a row
  constexpr bool LEAN = vjp_lean_trig<T>();
  static_assert(!M::HAS_LUT, "no reverse mode for the saturated PMSM");
  extern __shared__ __attribute__((aligned(16))) unsigned char policy_vjp_lds[];
  const int64_t blk0 = (int64_t)blockIdx.x * BLK;  // first environment of the workgroup
  const unsigned lane0 = threadIdx.x;
  unsigned lane = lane0;  // refreshed per row, as in sim_ahead_vjp_kernel: (uniform pointer + uniform offset) + one 32-bit lane offset
  const int64_t B = ka.B;
  if (blk0 + lane0 >= B) return;  // (no barrier below)
  const int32_t K = (int32_t)ka.K, N = K * ka.substeps;  // (host: N fits)
  const int64_t OW = O + ka.n_control;
  const int L = ka.n_layers;
  const int activation = ka.activation;
  // this lane's LDS column: hidden layer l (1 .. L - 1), unit j at hcol[(hoff_l + j) * BLK], hoff_l = d_1 + .. + d_{l-1}
  T* const hcol = reinterpret_cast<T*>(policy_vjp_lds) + threadIdx.x;
  Ctx<T, M> c;
  load_ctx<false>(c, ka.kp, 0, ka.dt, ka.env_tau, ka.adv_coef);
  c.lin_stop = T(0);  // the trajectory clock of EXCENV_SEM_AHEAD: not read by a step
  c.lin_div = T(1);
  c.lin_last = 0;
  if constexpr (M::S >= 4 || M::IS_PMSM) {  // as sim_feedback_vjp_kernel: the refined reciprocals to scalar registers
#pragma unroll
    for (int j = 0; j < S; ++j) c.nrm[j].y = vjp_uniform(c.nrm[j].y);
#pragma unroll
    for (int j = 0; j < (M::ND > 0 ? M::ND : 1); ++j) c.den[j].y = vjp_uniform(c.den[j].y);
  }

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
  // the stored observation row n: the O observation columns and the n_control reference columns behind them
  auto load_obs_row = [&](int64_t n, T (&ob)[O], T (&cr)[NC]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < O; ++q) ob[q] = ((ka.obs + ((n * OW + q) * B + blk0)) + lane)[0];
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (j < ka.n_control) cr[j] = ((ka.obs + ((n * OW + O + j) * B + blk0)) + lane)[0];
  };

  T sb[S], ab[A];  // cotangents of the carried state and of the held action
  T om_c = T(0);   // PMSM: omega_el is a constant of the trajectory — row 0's value stands for every row's (same bits)
  if constexpr (M::IS_PMSM) om_c = ((ka.straj[6] + blk0) + lane)[0];
#pragma unroll
  for (int q = 0; q < A; ++q) ab[q] = T(0);
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
    T ga[A], ob[O], cref[NC];  // the grad_actions row of k and the stored observation row n - 1
    unsigned rst = 0;          // step n - 1 was a reset (substeps == 1: row n - 1 is the action row k)
#pragma unroll
    for (int q = 0; q < A; ++q) ga[q] = T(0);
#pragma unroll
    for (int q = 0; q < O; ++q) ob[q] = T(0);
#pragma unroll
    for (int j = 0; j < NC; ++j) cref[j] = T(0);
    auto load_policy_rows = [&]() __attribute__((always_inline)) {
      if (act) {
        if (ka.g_actions != nullptr) load_krow(ka.g_actions, k, ga);
        load_obs_row(n - 1, ob, cref);
        if (ka.reset != nullptr) rst = ((ka.reset + ((int64_t)k * B + blk0)) + lane)[0];
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
    // (with an episode mask omega_el is constant between two resets only: the row's own value — a reset step, where rows n - 1 and n
    // differ, is dropped below)
    if constexpr (M::IS_PMSM) s0[6] = s1[6] = (ka.reset != nullptr) ? svc[6] : om_c;
    T g0[A], g1[A];
    {
      T geps0 = T(0);
      env_step_vjp<M, SOLVER, false>(s0, s1, ac, ac, 0, 0, c, T(0), sb, geps0, g0, g1);
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
    // a reset step did not happen: what was accumulated for row n is dropped and the action of row n - 1 was written, not applied
    const bool dropped = rst != 0;
#pragma unroll
    for (int j = 0; j < S; ++j) sb[j] = dropped ? T(0) : sb[j];
#pragma unroll
    for (int q = 0; q < A; ++q) {
      const T gq = (SOLVER == EXCENV_EULER) ? g0[q] : g0[q] + g1[q];  // the c_i == 1 stages read the same row
      ab[q] = ab[q] + (dropped ? T(0) : gq);
    }
    if (act) {
      // the transposed policy at row n - 1: the clamp has derivative 0 on and outside its bounds, a NaN compares false
      T pre[A], obb[O];
#pragma unroll
      for (int q = 0; q < A; ++q) {
        const T abq = ab[q] + ga[q];
        pre[q] = (ac[q] > ka.clip_lo && ac[q] < ka.clip_hi) ? abq : T(0);
        ab[q] = T(0);
      }
#pragma unroll
      for (int q = 0; q < A; ++q) {
        const T tmp[1] = {pre[q]};
        store_stream<T, 1>((ka.g_raw + (((int64_t)k * A + q) * B + blk0)) + lane, tmp);
      }
#pragma unroll
      for (int o = 0; o < O; ++o) obb[o] = T(0);
      if (L == 1) {
        // no hidden layer: registers to registers
#pragma unroll
        for (int q = 0; q < A; ++q) {
          const T* w = params + q * (int)OW;
#pragma unroll
          for (int o = 0; o < O; ++o) obb[o] = xfma(w[o], pre[q], obb[o]);
        }
      } else {
        const int iOW = (int)OW;
        // ---- the forward's statements again, every hidden layer kept. Layer 1: registers to LDS
        const int d1 = ka.widths[1];
        {
          const T* bias = params + d1 * iOW;
          for (int j0 = 0; j0 < d1; j0 += JB) {
            T acc[JB];
#pragma unroll
            for (int r = 0; r < JB; ++r) {
              const int jr = (j0 + r < d1) ? j0 + r : d1 - 1;
              const T* w = params + jr * iOW;
              acc[r] = bias[jr];
#pragma unroll
              for (int o = 0; o < O; ++o) acc[r] = xfma(w[o], ob[o], acc[r]);
#pragma unroll
              for (int j = 0; j < NC; ++j)
                if (j < ka.n_control) acc[r] = xfma(w[O + j], cref[j], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < JB; ++r)
              if (j0 + r < d1) hcol[(j0 + r) * BLK] = policy_act(acc[r], activation);
          }
        }
        int off = d1 * (iOW + 1);  // where the next layer's parameters start
        int nin = d1;              // its input width
        int hin_off = 0;           // the LDS row of its first input
        // hidden layers 2 .. L - 1: LDS to LDS
#pragma unroll
        for (int l = 2; l < EXCENV_POLICY_MAX_LAYERS; ++l) {
          if (l < L) {
            const int d = ka.widths[l];
            const T* hin = hcol + hin_off * BLK;
            T* hout = hcol + (hin_off + nin) * BLK;
            const T* bias = params + off + d * nin;
            for (int j0 = 0; j0 < d; j0 += JB) {
              T acc[JB];
              const T* w[JB];
#pragma unroll
              for (int r = 0; r < JB; ++r) {
                const int jr = (j0 + r < d) ? j0 + r : d - 1;
                w[r] = params + off + jr * nin;
                acc[r] = bias[jr];
              }
#pragma unroll UNR
              for (int m = 0; m < nin; ++m) {
                const T x = hin[m * BLK];
#pragma unroll
                for (int r = 0; r < JB; ++r) acc[r] = xfma(w[r][m], x, acc[r]);
              }
#pragma unroll
              for (int r = 0; r < JB; ++r)
                if (j0 + r < d) hout[(j0 + r) * BLK] = policy_act(acc[r], activation);
            }
            off += d * (nin + 1);
            hin_off += nin;
            nin = d;
          }
        }
        // here: `off` is where W_L starts, x^{L-1} (nin units) sits at LDS row hin_off
        // ---- the transposed output layer: registers (pre) to LDS, d^{L-1} over x^{L-1} in place
        {
          T* hx = hcol + hin_off * BLK;
          for (int i0 = 0; i0 < nin; i0 += UNR) {
            T xb[UNR];
#pragma unroll
            for (int r = 0; r < UNR; ++r) xb[r] = T(0);
#pragma unroll
            for (int q = 0; q < A; ++q) {
              const T* w = params + off + q * nin;
#pragma unroll
              for (int r = 0; r < UNR; ++r) {
                const int ir = (i0 + r < nin) ? i0 + r : nin - 1;
                xb[r] = xfma(w[ir], pre[q], xb[r]);
              }
            }
#pragma unroll
            for (int r = 0; r < UNR; ++r)
              if (i0 + r < nin) hx[(i0 + r) * BLK] = policy_act_vjp(xb[r], hx[(i0 + r) * BLK], activation);
          }
        }
        // ---- the transposed hidden layers L - 1 .. 2: LDS (d^l) to LDS (d^{l-1} over x^{l-1} in place)
#pragma unroll
        for (int l = EXCENV_POLICY_MAX_LAYERS - 1; l >= 2; --l) {
          if (l < L) {
            const int d = nin;             // outputs of layer l: d^l sits at LDS row hin_off
            const int ni = ka.widths[l - 1];  // its inputs
            off -= d * (ni + 1);           // where W_l starts
            const T* hd = hcol + hin_off * BLK;
            T* hx = hcol + (hin_off - ni) * BLK;
            const T* wl = params + off;
            for (int i0 = 0; i0 < ni; i0 += UNR) {
              T xb[UNR];
              int ir[UNR];
#pragma unroll
              for (int r = 0; r < UNR; ++r) {
                xb[r] = T(0);
                ir[r] = (i0 + r < ni) ? i0 + r : ni - 1;
              }
#pragma unroll 2
              for (int j = 0; j < d; ++j) {
                const T dj = hd[j * BLK];
                const T* w = wl + j * ni;
#pragma unroll
                for (int r = 0; r < UNR; ++r) xb[r] = xfma(w[ir[r]], dj, xb[r]);
              }
#pragma unroll
              for (int r = 0; r < UNR; ++r)
                if (i0 + r < ni) hx[(i0 + r) * BLK] = policy_act_vjp(xb[r], hx[(i0 + r) * BLK], activation);
            }
            hin_off -= ni;
            nin = ni;
          }
        }
        // ---- the transposed layer 1: LDS (d^1) to registers, the O observation columns only (references get no gradient)
        {
          const T* hd = hcol;  // (hin_off == 0, nin == d1)
#pragma unroll 2
          for (int j = 0; j < d1; ++j) {
            const T dj = hd[j * BLK];
            const T* w = params + j * iOW;
#pragma unroll
            for (int o = 0; o < O; ++o) obb[o] = xfma(w[o], dj, obb[o]);
          }
        }
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
}

// Packs PolicyVjpArgs and enqueues the one launch of a call on the call's stream
template <class M, typename T> static int launch_policy_vjp(const PolicyVjpCall& vc) {
  const char* fn = "excenv_sim_policy_vjp";
  PolicyVjpArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  if (int rc = reverse_preamble(fn, ka, vc.props, vc.obs_stepsize, vc.env_tau, false)) return rc;
  const excenv_policy_vjp_t& r = *vc.r;
  const excenv_policy_t& p = r.policy;
  ka.B = vc.B;
  ka.K = vc.K;
  ka.substeps = vc.substeps;
  ka.n_control = vc.control ? vc.control->n_control : 0;
  for (int j = 0; j < M::S; ++j) {
    if (!r.state_traj[j] || !r.grad_state0[j]) { set_error("%s: state pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    ka.straj[j] = (const T*)r.state_traj[j];
    ka.g_straj[j] = r.grad_states ? (const T*)r.grad_states[j] : nullptr;
    ka.g_last[j] = r.grad_last_state ? (const T*)r.grad_last_state[j] : nullptr;
    ka.g_state0[j] = (T*)r.grad_state0[j];
  }
  ka.obs = (const T*)r.obs_traj;
  ka.actions = (const T*)r.actions;
  ka.reset = r.reset;
  ka.n_layers = p.n_layers;
  ka.activation = p.activation;
  for (int l = 0; l <= p.n_layers; ++l) ka.widths[l] = p.widths[l];
  ka.g_obs = (const T*)r.grad_obs;
  ka.g_actions = (const T*)r.grad_actions;
  ka.g_raw = (T*)r.grad_raw;
  ka.clip_lo = (T)p.clip_lo;
  ka.clip_hi = (T)p.clip_hi;
  if (vc.B == 0) return EXCENV_OK;
  const int64_t blocks = (vc.B + POLICY_BLOCK - 1) / POLICY_BLOCK;
  if (blocks > (int64_t)0x7fffffff) {
    set_error("%s: ceil(B / %d) = %lld workgroups exceed one launch", fn, POLICY_BLOCK, (long long)blocks);
    return EXCENV_EINVAL;
  }
  const dim3 grid((unsigned)blocks), block(POLICY_BLOCK);
  const size_t lds = policy_vjp_lds_bytes(p, sizeof(T));
  const hipStream_t stream = (hipStream_t)vc.stream;
  const T* params = (const T*)p.params;
  with_solver(vc.solver, [&](auto solver) {  // (check_common has validated the id)
    launch_dyn(sim_policy_vjp_kernel<M, T, decltype(solver)::value>, grid, block, lds, stream, ka, params);
    return true;
  });
  g_last_launch = policy_vjp_name();
  return check_launch(fn);
}

// EnvVTable::sim_policy_vjp (launch.hpp): a model's translation unit policy_vjp_<model>.hip instantiates it
template <template <typename> class MT> int policy_vjp_entry(const PolicyVjpCall& vc) {
  if constexpr (MT<float>::HAS_LUT) {
    set_error("excenv_sim_policy_vjp: the saturated PMSM (pmsm_lut) has no reverse mode");
    return EXCENV_EUNSUPPORTED;
  } else {
    return EXCENV_BY_DTYPE(launch_policy_vjp, MT, vc);
  }
}

}  // namespace excenv
