// Episode rollouts: sim_episodes_kernel is sim_policy_kernel (kernels_policy.hpp) with the gym outputs of every saved row and the
// episode boundaries inside the launch (include/excenv.h excenv_episode_t). One solver step per action (N = K). On the
// row just saved, per environment:
//   truncated[n] = generate_truncated(st_n);  n >= 1: reward[n-1], terminated[n-1] = generate_reward / generate_terminated(st_n)
//   a[n] = the policy of sim_policy_kernel (policy_mlp), stored in every case
//   end_n = (end_mask & 1 and terminated) or (end_mask & 2 and any truncated) or (max_episode_steps > 0 and t >= max_episode_steps)
//   st_{n+1} = end_n ? reset_states[e mod R] : env_step(st_n, a[n])
// Reward and terminated are gym_outputs' (kernels.hpp), the function the step and the general trajectory kernels call, on registers;
// the per-column truncated flags are packed into words as the lean trajectory kernel packs them: the same bits as a second pass over
// the state trajectory. Every lane steps; a lane whose episode has ended then loads its reset row under its
// own (divergent) branch and the two states are blended by a select, so a launch without resets reads no reset row. e mod R is a
// wrapped counter. The saturated model looks its table values up again at a reset state. The two "is this output wanted" questions
// are launch-uniform: an output that is NULL and feeds no end condition costs nothing.
//   One wavefront per workgroup, no barrier, no inline assembly, no scratch; dynamic LDS as sim_policy_kernel. Instantiated in
// policy_episodes_<model>.hip only.
#pragma once
#include "kernels_policy.hpp"

namespace excenv {

// sim_policy_kernel's network as a function (the same statements; that kernel keeps them inline so that its code stays as it was):
// x^L of the network on one observation row (`ob`, then the first n_control entries of `cref`), in the contract's order: the first
// layer reads registers, hidden layers ping-pong through this lane's LDS column `hcol` (buffers of `hbuf` elements), the last one
// accumulates into y[]. `params` as the kernel argument: wave-uniform indices, so the loads are scalar.
template <class M, typename T>
__device__ __forceinline__ void policy_mlp(const PolicyArgs<T, M>& ka, const T* __restrict__ params, const T (&ob)[M::O],
                                           const T (&cref)[EXCENV_MAX_CONTROL], T* const hcol, const int hbuf, const int OW, const int L,
                                           const int activation, T (&y)[M::A]) {
  constexpr int A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL, BLK = POLICY_BLOCK, JB = POLICY_JB;
  constexpr int UNR = 32 / (int)sizeof(T);  // inputs per unrolled pass: 8 (fp32) or 4 (fp64) consecutive weights of a row at once
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
}

template <typename T, class M> struct EpisodeArgs {
  PolicyArgs<T, M> p;
  const T* reset_states[M::S];  // [R][B] each
  int32_t n_reset_rows, end_mask, max_episode_steps;
  int32_t trunc_words;  // truncated is 4-byte aligned: an even TW leaves as words (store_flag_bytes), else byte by byte
  const int32_t* steps_in;  // [B] or nullptr
  T* reward;                // [K][B]
  uint8_t* terminated;      // [K][B]
  uint8_t* truncated;       // [K + 1][B][TW]
  uint8_t* reset;           // [K][B]
  int32_t* n_resets;        // [B]
  int32_t* steps_out;       // [B]
};

template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(POLICY_BLOCK) __attribute__((amdgpu_waves_per_eu(policy_min_waves<M, T, SOLVER>())))
sim_episodes_kernel(const EpisodeArgs<T, M> ea, const T* __restrict__ params) {
  constexpr int S = M::S, A = M::A, O = M::O, NC = EXCENV_MAX_CONTROL, BLK = POLICY_BLOCK;
  constexpr bool ONE_FLAG = M::IS_PMSM || M::ID == EXCENV_FLUID_TANK;  // TW == 1
  constexpr int NWM = ONE_FLAG ? 1 : (O + NC + 3) / 4;  // the truncated flags of a row, one byte each, as words
  const PolicyArgs<T, M>& ka = ea.p;
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
  T memo[1][6];  // look-up model: the table values at the current operating point
  if constexpr (M::HAS_LUT) M::lookup(st[3], st[4], c, memo[0]);

  // reference-tracking columns and the physical references of the reward: constant along the call (a reset does not redraw them)
  T cref[NC], rref[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    cref[j] = rref[j] = T(0);
    if (j < ka.n_control) {
      const int f = ka.control_idx[j];
      T lo = c.smin[0], hi = c.smax[0];
#pragma unroll
      for (int q = 1; q < S; ++q) {
        lo = (f == q) ? c.smin[q] : lo;
        hi = (f == q) ? c.smax[q] : hi;
      }
      rref[j] = ka.reference[j][i];
      cref[j] = normalize(rref[j], lo, hi);
    }
  }

  // ... and so are the truncated flags of the control columns: byte O + j of a row's flags
  uint32_t cw[NWM];
#pragma unroll
  for (int q = 0; q < NWM; ++q) cw[q] = 0u;
  if constexpr (!ONE_FLAG) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (j < ka.n_control) cw[(O + j) >> 2] |= (xabs(cref[j]) > T(1)) ? (1u << (((O + j) & 3) * 8)) : 0u;
  }

  const int OW = O + ka.n_control;
  const int TW = ONE_FLAG ? 1 : OW;
  const int L = ka.n_layers;
  const int activation = ka.activation;
  T* const hcol = reinterpret_cast<T*>(policy_lds) + threadIdx.x;
  const int hbuf = ka.hw * BLK;

  const int64_t K = ka.K;
  const bool with_states = ka.straj[0] != nullptr;
  const int64_t o_row = (int64_t)OW * ka.B;
  T* orow = ka.obs + i;
  int64_t s_off = i;  // n * B + i

  // what a row has to compute (launch-uniform): reward and terminated come together (terminated is `reward == 0` for five models)
  const bool end_term = (ea.end_mask & EXCENV_END_TERMINATED) != 0, end_trunc = (ea.end_mask & EXCENV_END_TRUNCATED) != 0;
  const bool need_rt = ea.reward != nullptr || ea.terminated != nullptr || end_term;
  const bool need_tr = ea.truncated != nullptr || end_trunc;
  const int32_t tmax = ea.max_episode_steps;
  const int32_t R = ea.n_reset_rows;
  int32_t t = ea.steps_in != nullptr ? ea.steps_in[i] : 0;
  int32_t e = 0, er = 0;  // resets so far, and e mod R

  const bool with_noise = ka.noise != nullptr && K > 0;
  const int64_t klast = K - 1;
  T nzc[A], nzn[A];
#pragma unroll
  for (int q = 0; q < A; ++q) nzc[q] = nzn[q] = with_noise ? ka.noise[q * ka.B + i] : T(0);

  for (int64_t n = 0;; ++n) {
    // the noise row of action n + 1 is requested before row n is saved (kernels_policy.hpp)
    if (n < K && with_noise) {
      const int64_t k1 = (n < klast) ? n + 1 : klast;
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
    // ---- its gym outputs, in registers: reward and terminated from gym_outputs; the truncated flags of the models that have one per
    // observation column are packed as the lean trajectory kernel packs them (|obs| > 1 per column next to the constant flags of the
    // control columns), which is what gym_outputs stores byte by byte
    T rew = T(0);
    uint8_t te = 0, tr0 = 0;
    uint32_t tw[NWM];
#pragma unroll
    for (int q = 0; q < NWM; ++q) tw[q] = cw[q];
    if constexpr (ONE_FLAG) {
      if (need_rt) gym_outputs<M, T>(st, ob, c, ka.n_control, ka.control_idx, rref, &rew, &te, &tr0, 1);
      else if (need_tr) gym_outputs<M, T>(st, ob, c, ka.n_control, ka.control_idx, rref, nullptr, nullptr, &tr0, 1);
      tw[0] = tr0;
    } else {
      if (need_rt) gym_outputs<M, T>(st, ob, c, ka.n_control, ka.control_idx, rref, &rew, &te, nullptr, 1);
      if (need_tr) {
#pragma unroll
        for (int q = 0; q < O; ++q) tw[q >> 2] |= (xabs(ob[q]) > T(1)) ? (1u << ((q & 3) * 8)) : 0u;
      }
    }
    if (ea.truncated != nullptr) {
      uint8_t* tp = ea.truncated + s_off * TW;
      if constexpr (ONE_FLAG) {
        tp[0] = tr0;
      } else {
        dispatch_count<0, NC>(ka.n_control, [&](auto tag) {
          constexpr int TWc = O + decltype(tag)::value, NW = (TWc + 3) / 4;
          bool stored = false;
          if constexpr (TWc % 2 == 0) {  // an environment's flags as one store where their width and the base allow it
            if (ea.trunc_words) {
              uint32_t w[NW];
#pragma unroll
              for (int q = 0; q < NW; ++q) w[q] = tw[q];
              store_flag_bytes<TWc>(tp, w);
              stored = true;
            }
          }
          if (!stored) {
#pragma unroll
            for (int q = 0; q < TWc; ++q) tp[q] = (uint8_t)(tw[q >> 2] >> ((q & 3) * 8));
          }
        });
      }
    }
    if (n > 0) {
      if (ea.reward != nullptr) {
        const T tmp[1] = {rew};
        store_stream<T, 1>(ea.reward + (s_off - ka.B), tmp);
      }
      if (ea.terminated != nullptr) ea.terminated[s_off - ka.B] = te;
    }
    orow += o_row;
    if (n == K) break;
    // ---- the policy on the row just saved: computed and stored in every case
    T a[A];
    {
      T y[A];  // x^L
      policy_mlp<M, T>(ka, params, ob, cref, hcol, hbuf, OW, L, activation, y);
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
          store_stream<T, 1>(ka.actions_out + (n * A + q) * ka.B + i, tmp);
        }
      }
    }
    // ---- has the episode ended on this row?
    bool end = end_term && te != 0;
    if (end_trunc) {
#pragma unroll
      for (int q = 0; q < NWM; ++q) end = end || tw[q] != 0u;
    }
    end = end || (tmax > 0 && t >= tmax);
    if (ea.reset != nullptr) ea.reset[s_off] = end ? 1 : 0;
    // ---- step n under the action; a lane at an episode end takes its reset row instead
    T nx[S];
#pragma unroll
    for (int j = 0; j < S; ++j) nx[j] = st[j];
    env_step<M, SOLVER>(nx, a, c, M::HAS_LUT ? &memo[0] : nullptr);
    T rs[S];
#pragma unroll
    for (int j = 0; j < S; ++j) rs[j] = T(0);
    if (end) {
      const int64_t r_off = (int64_t)er * ka.B + i;
#pragma unroll
      for (int j = 0; j < S; ++j) rs[j] = ea.reset_states[j][r_off];
      // s_waitcnt vmcnt(0), here: the memory counter is in order, so waiting for these loads drains the row's stores. Left to the
      // compiler, the wait sits behind the join, at the first use of the blended state, where every lane of every row pays for it
      // whether or not anything was loaded, and the noise row in flight is waited for with it (B = 2^15, K = 1000, 16 hidden units:
      // pendulum 8.48 -> 8.06 ms, PMSM 7.64 -> 7.36 ms); here only a wave with an episode end does.
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
#pragma unroll
    for (int j = 0; j < S; ++j) st[j] = end ? rs[j] : nx[j];
    if constexpr (M::HAS_LUT) {
      if (end) M::lookup(st[3], st[4], c, memo[0]);  // the new operating point
    }
    er = end ? ((er + 1 == R) ? 0 : er + 1) : er;
    e += end ? 1 : 0;
    t = end ? 0 : t + 1;
    s_off += ka.B;
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const T tmp[1] = {st[j]};
    store_v<T, 1>(ka.last_state[j] + i, tmp);
  }
  if (ea.n_resets != nullptr) ea.n_resets[i] = e;
  if (ea.steps_out != nullptr) ea.steps_out[i] = t;
}

// Packs EpisodeArgs and launches the instantiation of the call's solver
template <class M, typename T> static int launch_episodes(const EpisodeCall& ec) {
  const PolicyCall& pc = ec.call;
  const excenv_episode_t& ep = *ec.episode;
  EpisodeArgs<T, M> ea;
  std::memset(&ea, 0, sizeof(ea));
  int64_t blocks;
  if (int rc = pack_policy_args<M, T>("excenv_sim_policy_episodes", pc, ea.p, &blocks)) return rc;
  for (int j = 0; j < M::S; ++j) ea.reset_states[j] = (const T*)ep.reset_states[j];  // (episode_refusal has seen every leaf)
  ea.n_reset_rows = ep.n_reset_rows;
  ea.end_mask = ep.end_mask;
  ea.max_episode_steps = ep.max_episode_steps;
  ea.trunc_words = ((uintptr_t)ep.truncated % 4) == 0;
  ea.steps_in = ep.episode_steps_in;
  ea.reward = (T*)ep.reward;
  ea.terminated = ep.terminated;
  ea.truncated = ep.truncated;
  ea.reset = ep.reset;
  ea.n_resets = ep.n_resets;
  ea.steps_out = ep.episode_steps_out;
  if (pc.B == 0) return EXCENV_OK;
  const dim3 grid((unsigned)blocks), block(POLICY_BLOCK);
  const size_t lds = policy_lds_bytes(*pc.policy, sizeof(T));
  const hipStream_t stream = (hipStream_t)pc.stream;
  const T* params = (const T*)pc.policy->params;
  with_solver(pc.solver, [&](auto solver) {  // (check_common has validated the id)
    hipLaunchKernelGGL((sim_episodes_kernel<M, T, decltype(solver)::value>), grid, block, lds, stream, ea, params);
    return true;
  });
  g_last_launch = episodes_name();
  return check_launch("excenv_sim_policy_episodes");
}

// EnvVTable::sim_policy_episodes (launch.hpp): a model's translation unit policy_episodes_<model>.hip instantiates it
template <template <typename> class MT> int policy_episodes_entry(const EpisodeCall& ec) {
  return ec.call.dtype == EXCENV_F32 ? launch_episodes<MT<float>, float>(ec) : launch_episodes<MT<double>, double>(ec);
}

}  // namespace excenv
