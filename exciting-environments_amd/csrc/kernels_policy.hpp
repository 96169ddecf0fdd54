// Policy rollouts: sim_policy_kernel is sim_feedback_kernel (kernels_feedback.hpp) with a small multi-layer perceptron in place of the
// gain block (include/excenv.h excenv_policy_t). At every action row, on the observation row just saved:
//   x^0 = obs_n;  x^l[j] = act(b_l[j] + sum_i W_l[j][i] x^{l-1}[i])  (fused multiply-adds in the order of i);  x^L without act
//   a[k][q] = clamp(noise[k][q] + x^L[q], lo, hi)
// The loop around it is the one-environment-per-lane general form of sim_ahead_body.inc under EXCENV_SEM_STEP, so a trajectory is
// bit for bit what the open-loop kernel returns for the applied actions.
//   Where things live. The parameters are shared by all environments: they are read through wave-uniform indices from a
// `const T* __restrict__` kernel argument, so the loads are scalar and the weights are scalar operands of the FMAs; nothing is staged
// per lane. Hidden activations cannot be a register array (the widths are run-time values: it would go to scratch), so a lane keeps
// them in its own LDS column h[buf][j][lane], ping-ponged between layers: consecutive lanes hit consecutive banks, and a lane only
// reads what it wrote itself, so there is no barrier anywhere. The first layer reads ob[] / cref[] from registers, the last one
// accumulates into A registers. POLICY_JB outputs are computed per pass so that one activation read feeds POLICY_JB FMAs; each output
// still sums in the order of i. A tail block recomputes the last row instead of branching and skips the stores.
//   One wavefront per workgroup (policy.hpp POLICY_BLOCK); the dynamic LDS is sized by the call's widest hidden layer. The activation
// is a launch-uniform branch. No inline assembly, no scratch. Instantiated in policy_<model>.hip only.
#pragma once
#include "launch.hpp"
#include "policy.hpp"

namespace excenv {

constexpr int POLICY_JB = 4;  // outputs per pass over a layer's inputs

template <typename T, class M> struct PolicyArgs {
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
  int32_t n_layers, activation;
  int32_t widths[EXCENV_POLICY_MAX_LAYERS + 1];
  int32_t hw;          // rows of one LDS buffer: the widest hidden layer
  const T* noise;      // [K][A][B] or nullptr
  T* actions_out;      // [K][A][B] or nullptr
  T clip_lo, clip_hi;  // max_nan / min_nan (a NaN passes through); -inf / +inf change nothing
  T dt, env_tau, adv_coef;
};

__device__ __forceinline__ float policy_tanh(float x) { return ::tanhf(x); }
__device__ __forceinline__ double policy_tanh(double x) { return ::tanh(x); }

template <typename T> __device__ __forceinline__ T policy_act(T y, int activation) {
  if (activation == EXCENV_ACT_TANH) return policy_tanh(y);
  return (y < T(0)) ? T(0) : y;
}

// The register caps of sim_feedback_kernel (kernels_feedback.hpp) without its gain registers: the general trajectory kernel's
template <class M, typename T, int SOLVER> constexpr int policy_min_waves() { return sim_min_waves<M, T, true, false, false, -2, SOLVER>(); }

extern __shared__ __attribute__((aligned(16))) unsigned char policy_lds[];

template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(POLICY_BLOCK) __attribute__((amdgpu_waves_per_eu(policy_min_waves<M, T, SOLVER>())))
sim_policy_kernel(const PolicyArgs<T, M> ka, const T* __restrict__ params) {
  constexpr int S = M::S, A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL, BLK = POLICY_BLOCK, JB = POLICY_JB;
  constexpr int UNR = 32 / (int)sizeof(T);  // inputs per unrolled pass: 8 (fp32) or 4 (fp64) consecutive weights of a row at once
  const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  Ctx<T, M> c;
  load_ctx<true>(c, ka.kp, (i < ka.B) ? i : 0, ka.dt, ka.env_tau, ka.adv_coef);  // lut_lds = 0: the tables stay in global memory
  c.lin_stop = T(0);  // the trajectory clock of EXCENV_SEM_AHEAD: not read by a step
  c.lin_div = T(1);
  c.lin_last = 0;
  if (i >= ka.B) return;  // (no barrier below)

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

  const int OW = O + ka.n_control;
  const int L = ka.n_layers;
  const int activation = ka.activation;
  // this lane's LDS column: buffer b, row j at hcol[(b * hw + j) * BLK]
  T* const hcol = reinterpret_cast<T*>(policy_lds) + threadIdx.x;
  const int hbuf = ka.hw * BLK;

  const int64_t N = ka.K * ka.substeps;
  const bool with_states = ka.straj[0] != nullptr;
  const int64_t o_row = (int64_t)OW * ka.B;
  T* orow = ka.obs + i;
  int64_t s_off = i;

  // the noise row of action k, and the next one in flight
  const bool with_noise = ka.noise != nullptr && ka.K > 0;
  const int64_t klast = ka.K - 1;
  T nzc[A], nzn[A];
#pragma unroll
  for (int q = 0; q < A; ++q) nzc[q] = nzn[q] = with_noise ? ka.noise[q * ka.B + i] : T(0);

  T a[A];
#pragma unroll
  for (int q = 0; q < A; ++q) a[q] = T(0);
  int64_t k = 0;
  int32_t sub = 0;
  for (int64_t n = 0;; ++n) {
    const bool act = sub == 0 && n < N;  // row n is an action row (wave-uniform)
    // row k + 1 of the noise is requested before row n is saved and step n is computed, and first read one action later; the index
    // is clamped, so the load is unconditional (DESIGN.md §4.1 "Pipeline")
    if (act && with_noise) {
      const int64_t k1 = (k < klast) ? k + 1 : klast;
#pragma unroll
      for (int q = 0; q < A; ++q) nzn[q] = ka.noise[(k1 * A + q) * ka.B + i];
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
      T y[A];  // x^L
      if (L == 1) {
        // no hidden layer: registers to registers
#pragma unroll
        for (int q = 0; q < A; ++q) {
          const T* w = params + q * OW;
          T acc = params[A * OW + q];
#pragma unroll
          for (int o = 0; o < O; ++o) acc = xfma(w[o], ob[o], acc);
#pragma unroll
          for (int j = 0; j < NC; ++j)
            if (j < ka.n_control) acc = xfma(w[O + j], cref[j], acc);
          y[q] = acc;
        }
      } else {
        // layer 1: registers to LDS buffer 0
        const int d1 = ka.widths[1];
        {
          const T* bias = params + d1 * OW;
          for (int j0 = 0; j0 < d1; j0 += JB) {
            T acc[JB];
#pragma unroll
            for (int r = 0; r < JB; ++r) {
              const int jr = (j0 + r < d1) ? j0 + r : d1 - 1;
              const T* w = params + jr * OW;
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
        int off = d1 * (OW + 1);  // where the next layer's parameters start
        int nin = d1;             // its input width
        int cur = 0;              // the LDS buffer that holds its inputs
        // hidden layers 2 .. L - 1: LDS to LDS
#pragma unroll
        for (int l = 2; l < EXCENV_POLICY_MAX_LAYERS; ++l) {
          if (l < L) {
            const int d = ka.widths[l];
            const T* hin = hcol + cur * hbuf;
            T* hout = hcol + (cur ^ 1) * hbuf;
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
            nin = d;
            cur ^= 1;
          }
        }
        // the output layer: LDS to registers
        {
          const T* hin = hcol + cur * hbuf;
          const T* bias = params + off + A * nin;
#pragma unroll
          for (int q = 0; q < A; ++q) y[q] = bias[q];
#pragma unroll UNR
          for (int m = 0; m < nin; ++m) {
            const T x = hin[m * BLK];
#pragma unroll
            for (int q = 0; q < A; ++q) y[q] = xfma(params[off + q * nin + m], x, y[q]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < A; ++q) {
        const T raw = with_noise ? nzc[q] + y[q] : y[q];
        a[q] = min_nan(max_nan(raw, ka.clip_lo), ka.clip_hi);
        nzc[q] = nzn[q];
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
}

// Packs PolicyArgs from a validated call, under the entry point's name `fn`; `blocks`: the workgroups of its launch
template <class M, typename T> static int pack_policy_args(const char* fn, const PolicyCall& pc, PolicyArgs<T, M>& ka, int64_t* blocks) {
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, pc.props);
  double coef;
  if (int rc = pmsm_coef<M>(pc.props, pc.env_tau, &coef)) return rc;
  ka.B = pc.B;
  ka.K = pc.K;
  ka.substeps = pc.substeps;
  ka.n_control = pc.control ? pc.control->n_control : 0;
  for (int j = 0; j < M::S; ++j) {
    if (!pc.state_in[j] || !pc.last_state[j]) { set_error("%s: state pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    if (pc.state_traj && !pc.state_traj[j]) { set_error("%s: state_traj pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    ka.state_in[j] = (const T*)pc.state_in[j];
    ka.last_state[j] = (T*)pc.last_state[j];
    ka.straj[j] = pc.state_traj ? (T*)pc.state_traj[j] : nullptr;
  }
  ka.obs = (T*)pc.obs_traj;
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = pc.control->control_idx[j];
    ka.reference[j] = (const T*)pc.control->reference[j];
  }
  const excenv_policy_t& p = *pc.policy;
  ka.n_layers = p.n_layers;
  ka.activation = p.activation;
  for (int l = 0; l <= p.n_layers; ++l) ka.widths[l] = p.widths[l];
  ka.hw = policy_widest_hidden(p);
  ka.noise = (const T*)p.noise;
  ka.actions_out = (T*)pc.actions_out;
  ka.clip_lo = (T)p.clip_lo;
  ka.clip_hi = (T)p.clip_hi;
  ka.dt = (T)pc.obs_stepsize;
  ka.env_tau = (T)pc.env_tau;
  ka.adv_coef = (T)coef;
  *blocks = (pc.B + POLICY_BLOCK - 1) / POLICY_BLOCK;
  if (*blocks > (int64_t)0x7fffffff) {
    set_error("%s: ceil(B / %d) = %lld workgroups exceed one launch", fn, POLICY_BLOCK, (long long)*blocks);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

// Launches the instantiation of the call's solver
template <class M, typename T> static int launch_policy(const PolicyCall& pc) {
  PolicyArgs<T, M> ka;
  int64_t blocks;
  if (int rc = pack_policy_args<M, T>("excenv_sim_policy", pc, ka, &blocks)) return rc;
  const excenv_policy_t& p = *pc.policy;
  if (pc.B == 0) return EXCENV_OK;
  const dim3 grid((unsigned)blocks), block(POLICY_BLOCK);
  const size_t lds = policy_lds_bytes(p, sizeof(T));
  const hipStream_t stream = (hipStream_t)pc.stream;
  const T* params = (const T*)p.params;
  with_solver(pc.solver, [&](auto solver) {  // (check_common has validated the id)
    hipLaunchKernelGGL((sim_policy_kernel<M, T, decltype(solver)::value>), grid, block, lds, stream, ka, params);
    return true;
  });
  g_last_launch = policy_name();
  return check_launch("excenv_sim_policy");
}

// EnvVTable::sim_policy (launch.hpp): a model's translation unit policy_<model>.hip instantiates it
template <template <typename> class MT> int policy_entry(const PolicyCall& pc) { return EXCENV_BY_DTYPE(launch_policy, MT, pc); }

}  // namespace excenv
