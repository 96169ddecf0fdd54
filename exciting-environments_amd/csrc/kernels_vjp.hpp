// Reverse mode of the trajectory kernel: one persistent launch computes the vector-Jacobian product of an excenv_sim_ahead call
// from the state rows that call saved. Same shape as the forward: a workgroup owns 256 * V adjacent environments
// for the whole trajectory, one lane per environment (V = 1) or 16 bytes per lane; rows stream from N down to 0.
// No LDS, no inline assembly; the per-step checkpoints are the saved rows themselves, so nothing is stored on the way.
#pragma once
#include "launch.hpp"
#include "vjp.hpp"

namespace excenv {

template <typename T, class M> struct VjpArgs {
  KProps<T, M> kp;
  int64_t B, K;
  int32_t substeps, n_control;
  const T* actions;         // [K][A][B]
  const T* straj[M::S];     // [N + 1][B]
  const T* g_obs;           // [N + 1][O + n_control][B] or nullptr
  const T* g_straj[M::S];   // [N + 1][B] or nullptr, per leaf
  const T* g_last[M::S];    // [B] or nullptr, per leaf
  T* g_actions;             // [K][A][B]
  T* g_state_in[M::S];      // [B]
  T dt, env_tau, adv_coef, lin_stop;
};
// The PGRAD instantiations' arguments: one [B] output per static-parameter leaf, nullptr where a leaf is not wanted
template <typename T, class M> struct VjpParamArgs : VjpArgs<T, M> {
  T* g_params[M::P];
};
template <typename T, class M, bool PGRAD> using VjpKernelArgs = std::conditional_t<PGRAD, VjpParamArgs<T, M>, VjpArgs<T, M>>;

// fp64: the reverse pass evaluates sin / cos with devmath.hpp's lean routine (registers and code size; the Jacobians move by
// rounding only), fp32 with the forward's own
template <typename T> constexpr bool vjp_lean_trig() { return sizeof(T) == 8; }
// ---- the register budget ------------------------------------------------------------------------------------------------------------
// Every instantiation runs at two waves per SIMD (amdgpu_waves_per_eu(2) on the kernel): 256 registers per lane, no scratch.
// tests/test_vjp_host.py checks both on the built library, and that check is the ONLY safety net for what follows: several of the
// helpers below work by keeping the optimiser from a transformation (common-subexpression elimination, hoisting) that is correct
// but costs registers. They change no value. Another compiler release may see through them or schedule differently, and the
// kernels would then spill silently — correct results, slower — until that test says so (DESIGN.md §4.9 "Register budget").

// x, as a value the optimiser cannot identify with x (an identity DPP move, folded into its user by the backend: no inline
// assembly). A stage state rebuilt from it in the reverse sweep is a NEW computation: without this, common-subexpression
// elimination hands the reverse sweep the forward pass's own stage states and every intermediate of f at them (sines, cosines,
// inertia terms of all stages), kept alive across the whole step — the opposite of what rebuilding is for.
__device__ __forceinline__ float vjp_opaque(float x) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xE4, 0xF, 0xF, false));
}
__device__ __forceinline__ double vjp_opaque(double x) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), 0xE4, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), 0xE4, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// A wave-uniform value the vector unit computed (the refined reciprocals of InvDiv: there is no scalar floating point), moved to
// scalar registers: left where they were computed, PMSM's nine reciprocals hold 18 vector registers in fp64 for the whole trajectory
__device__ __forceinline__ float vjp_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ double vjp_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
// The fp64 RK adjoints of the four-leaf models and PMSM rebuild the stage states from the slopes in the reverse sweep (from an
// opaque copy of the row) instead of keeping them
template <class M, typename T> constexpr bool vjp_rebuild_stages() { return sizeof(T) == 8 && (M::S == 4 || M::IS_PMSM); }
// A component of y that f neither reads nor feeds back into another (PMSM's angle: d eps / dt = omega_el): its Jacobian column is
// zero, so the stage cotangents of that component never change — spelled out, because x + a * 0 is not x to a compiler that must
// honour NaNs, and NS accumulators would stay in registers for nothing
template <class M> constexpr bool vjp_y_passive(int j) { return M::IS_PMSM && j == 2; }
// PMSM's wide form has no register to spare for the constants of the trajectory (initial angle, omega_el): it reads them again
// per row from row 0 (cache hits) instead of holding them
template <class M, int V> constexpr bool vjp_reload_constants() { return M::IS_PMSM && V > 1; }
// The cotangent rows of the next iteration are requested BEHIND the step's arithmetic instead of in front of it where their
// registers are needed during the step: in the fp64 RK instantiations that also rebuild their stages (a step there is hundreds of
// fp64 instructions; the second wave hides the latency) and in PMSM's wide form. PMSM in fp64 requests the saved row and the action
// row behind it as well (LATE_ROW in the kernel); everywhere else those two stay ahead of the arithmetic.
template <class M, typename T, int SOLVER, int V> constexpr bool vjp_late_cotangents() {
  return (SOLVER != EXCENV_EULER && vjp_rebuild_stages<M, T>()) || (M::IS_PMSM && V > 1);
}

// PGRAD: where the parameter accumulators live. The fp64 RK instantiations of the four-leaf models and PMSM (the ones that already
// rebuild their stages to stay within 256 registers; PMSM Tsit5 has one register to spare) have no room for P more fp64 values
// across the step: their accumulators sit in LDS, which the reverse kernel does not use otherwise — one private run of P | 1 elements
// per lane (an odd stride: the 32 lanes of a ds_read_b64 group hit distinct banks), added to in place by every transposed stage.
// Everywhere else they are registers. (Both this and the scheduling barriers of models.hpp are needed: either alone spills.)
template <class M, typename T, int SOLVER> constexpr bool vjp_pgrad_in_lds() { return SOLVER != EXCENV_EULER && vjp_rebuild_stages<M, T>(); }

// Adjoint of rk_step (rk.hpp) over Tableau<SOLVER>: recomputes the stage states from the step's starting point y0, then walks
// the stages in reverse. lam: in = cotangent of the step's result, out = cotangent of y0. ub / u1b: cotangents of the held action
// and of the action the c_i == 1 stages read (the caller routes u1b to the row that stage read). wb += cotangent of omega_el.
// PGRAD: every stage's transposed f also adds its parameter columns to pb[M::P].
template <class M, int SOLVER, bool PGRAD = false, typename T>
__device__ __forceinline__ void rk_step_vjp(const T (&y0)[M::NY], const T (&u)[M::A], const T (&u1)[M::A], const Ctx<T, M>& c,
                                            const T (&st)[M::S], T (&lam)[M::NY], T (&ub)[M::A], T (&u1b)[M::A], T& wb,
                                            T* pb = nullptr) {
  constexpr int NY = M::NY, A = M::A;
  constexpr bool LEAN = vjp_lean_trig<T>();
#pragma unroll
  for (int q = 0; q < A; ++q) ub[q] = u1b[q] = T(0);
  T fb[NY], yb[NY], tb[A];
  if constexpr (SOLVER == EXCENV_EULER) {
#pragma unroll
    for (int j = 0; j < NY; ++j) fb[j] = lam[j] * c.dt;
    if constexpr (PGRAD) M::template f_vjp<LEAN, true>(y0, u, c, st, fb, yb, tb, wb, pb);
    else M::template f_vjp<LEAN>(y0, u, c, st, fb, yb, tb, wb);
#pragma unroll
    for (int j = 0; j < NY; ++j) lam[j] = lam[j] + yb[j];
#pragma unroll
    for (int q = 0; q < A; ++q) ub[q] = tb[q];
  } else {
    using TB = Tableau<SOLVER>;
    constexpr int NS = TB::NS;
    // k_s = f(y_s) dt of all stages but the last, as rk_step evaluates them. The stage states y_s are kept for the reverse sweep or
    // (REBUILD: the large fp64 instantiations) rebuilt there from the slopes — NS * NY registers less for a few FMAs more. The
    // sums run over all NS slopes with the tableau's zeros skipped, so that every index is a constant once the loops are unrolled.
    constexpr bool REBUILD = vjp_rebuild_stages<M, T>();
    constexpr int NK = REBUILD ? 1 : NS;
    T k[NS][NY], yi[NK][NY], dy[NY];
#define EXCENV_STAGE_STATE(s, y, b)                                 \
  _Pragma("unroll") for (int j = 0; j < NY; ++j) {                 \
    T acc = T(0);                                                  \
    _Pragma("unroll") for (int q = 0; q < NS; ++q) {               \
      const T a = T(TB::a(s, q));                                  \
      if (q < s && a != T(0)) acc = xfma(a, k[q][j], acc);         \
    }                                                              \
    y[j] = (s == 0) ? b[j] : b[j] + acc;                           \
  }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      T (&y)[NY] = yi[REBUILD ? 0 : s];
      if (!REBUILD || s + 1 < NS) { EXCENV_STAGE_STATE(s, y, y0) }
      if (s + 1 < NS) {  // the last stage's slope is no stage state's input
        if (TB::c_is_one(s)) M::template f<LEAN>(y, u1, c, st, dy);
        else M::template f<LEAN>(y, u, c, st, dy);
#pragma unroll
        for (int j = 0; j < NY; ++j) k[s][j] = dy[j] * c.dt;
      }
    }
    T kb[NS][NY];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int j = 0; j < NY; ++j) kb[q][j] = T(TB::b(q)) * lam[j];
    T y0r[NY];  // REBUILD: the starting point as the reverse sweep sees it
#pragma unroll
    for (int j = 0; j < NY; ++j) y0r[j] = REBUILD ? vjp_opaque(y0[j]) : y0[j];
#pragma unroll
    for (int s = NS - 1; s >= 0; --s) {
      T (&y)[NY] = yi[REBUILD ? 0 : s];
      if (REBUILD) { EXCENV_STAGE_STATE(s, y, y0r) }
#pragma unroll
      for (int j = 0; j < NY; ++j) fb[j] = kb[s][j] * c.dt;
      if constexpr (PGRAD) {
        if (TB::c_is_one(s)) M::template f_vjp<LEAN, true>(y, u1, c, st, fb, yb, tb, wb, pb);
        else M::template f_vjp<LEAN, true>(y, u, c, st, fb, yb, tb, wb, pb);
      } else {
        if (TB::c_is_one(s)) M::template f_vjp<LEAN>(y, u1, c, st, fb, yb, tb, wb);
        else M::template f_vjp<LEAN>(y, u, c, st, fb, yb, tb, wb);
      }
#pragma unroll
      for (int j = 0; j < NY; ++j) {
        if (vjp_y_passive<M>(j)) continue;
        lam[j] = lam[j] + yb[j];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const T a = T(TB::a(s, q));
          if (q < s && a != T(0)) kb[q][j] = xfma(a, yb[j], kb[q][j]);
        }
      }
#pragma unroll
      for (int q = 0; q < A; ++q) {
        if (TB::c_is_one(s)) u1b[q] = u1b[q] + tb[q];
        else ub[q] = ub[q] + tb[q];
      }
    }
#undef EXCENV_STAGE_STATE
  }
}

// Adjoint of one solver step of one environment: env_advance_raw (AHEAD) or env_step (rk.hpp) from the saved row s0 to the saved
// row s1. sb: in = cotangent of the carried state after the step, out = before it. a / a1: the action rows k / k1 of the step;
// gk / gk1: their gradients' contributions (overwritten). PMSM under AHEAD carries more than the state: sb[0..1] is the cotangent of
// prev_clip (it moves back one row per step), sb[6] collects omega_el's, geps0 the initial angle's (every clip reads
// eps0 + t_k * omega_el). PGRAD: pb[M::P] += the step's parameter columns (post where the carried state is post-processed, every
// stage of the solver, every clip).
template <class M, int SOLVER, bool AHEAD, bool PGRAD = false, typename T>
__device__ __forceinline__ void env_step_vjp(const T (&s0)[M::S], const T (&s1)[M::S], const T (&a)[M::A], const T (&a1)[M::A],
                                             int64_t k, int64_t k1, const Ctx<T, M>& c, T eps0, T (&sb)[M::S], T& geps0,
                                             T (&gk)[M::A], T (&gk1)[M::A], T* pb = nullptr) {
  constexpr int NY = M::NY, A = M::A;
  constexpr bool LEAN = vjp_lean_trig<T>();
  if constexpr (PGRAD && !AHEAD) M::post_pvjp(s1, c, sb, pb);
  if constexpr (!AHEAD) M::post_vjp(s1, c, sb);  // the carried state is the post-processed one
  T y0[NY], lam[NY], u[A], u1[A], ub[A], u1b[A];
  T wb = T(0);
  M::get_y(s0, y0);
  M::get_y(sb, lam);
  if constexpr (!M::IS_PMSM) {
    u[0] = denormalize(a[0], c.amin[0], c.amax[0]);
    u1[0] = AHEAD ? denormalize(a1[0], c.amin[0], c.amax[0]) : u[0];
    rk_step_vjp<M, SOLVER, PGRAD>(y0, u, u1, c, s0, lam, ub, u1b, wb, pb);
    M::set_y(sb, lam);
    const T ds = T(0.5) * (c.amax[0] - c.amin[0]);  // d denormalize / d a
    gk[0] = ub[0] * ds;
    gk1[0] = u1b[0] * ds;
  } else {
    const bool dead = c.P[6] > T(0);
    const T om = s0[6];
    const T t_k = AHEAD ? ahead_time(k, c) : T(0), t_k1 = AHEAD ? ahead_time(k1, c) : T(0);
    const T ang = AHEAD ? eps0 + t_k * om : s0[2];
    const T ang1 = eps0 + t_k1 * om;
    constexpr bool NEXT_CLIP = AHEAD && SOLVER != EXCENV_EULER;  // a c_i == 1 stage reads the clip of row k1
    T uc[2];
    M::template constraint<LEAN>(a, ang, om, c, uc);
    if (dead) {  // the buffered voltage is the saved row's
      u[0] = s0[0];
      u[1] = s0[1];
      u1[0] = (AHEAD && k1 != k) ? uc[0] : u[0];
      u1[1] = (AHEAD && k1 != k) ? uc[1] : u[1];
    } else {
      u[0] = uc[0];
      u[1] = uc[1];
      u1[0] = u[0];
      u1[1] = u[1];
      if constexpr (NEXT_CLIP) M::template constraint<LEAN>(a1, ang1, om, c, u1);
    }
    rk_step_vjp<M, SOLVER, PGRAD>(y0, u, u1, c, s0, lam, ub, u1b, wb, pb);
    M::set_y(sb, lam);
    sb[6] = sb[6] + wb;
    T ucb[2], ucb1[2] = {T(0), T(0)};
    if (dead) {
      const bool own = !AHEAD || k1 == k;  // the c_i == 1 stage read the buffered voltage too
      ucb[0] = sb[0] + (own ? T(0) : u1b[0]);
      ucb[1] = sb[1] + (own ? T(0) : u1b[1]);
      sb[0] = ub[0] + (own ? u1b[0] : T(0));
      sb[1] = ub[1] + (own ? u1b[1] : T(0));
    } else if (NEXT_CLIP) {
      ucb[0] = ub[0];
      ucb[1] = ub[1];
      ucb1[0] = u1b[0];
      ucb1[1] = u1b[1];
    } else {
      ucb[0] = ub[0] + u1b[0];
      ucb[1] = ub[1] + u1b[1];
    }
    T eb = T(0), wc = T(0);
    gk[0] = gk[1] = gk1[0] = gk1[1] = T(0);
    // the transposed clip re-evaluates the clip at opaque copies of its inputs: identified with the evaluation above, its rotation,
    // sector and clamp intermediates would stay in registers across the whole RK adjoint
    const T ao[2] = {vjp_opaque(a[0]), vjp_opaque(a[1])};
    M::template constraint_vjp<LEAN, PGRAD>(ao, vjp_opaque(ang), om, c, ucb, gk, eb, wc, pb);
    if constexpr (AHEAD) {
      geps0 = geps0 + eb;
      sb[6] = sb[6] + (eb * t_k + wc);
    } else {
      sb[2] = sb[2] + eb;
      sb[6] = sb[6] + wc;
    }
    if constexpr (NEXT_CLIP) {
      if (!dead) {
        T eb1 = T(0), wc1 = T(0);
        const T a1o[2] = {vjp_opaque(a1[0]), vjp_opaque(a1[1])};
        M::template constraint_vjp<LEAN, PGRAD>(a1o, vjp_opaque(ang1), om, c, ucb1, gk1, eb1, wc1, pb);
        geps0 = geps0 + eb1;
        sb[6] = sb[6] + (eb1 * t_k1 + wc1);
      }
    }
  }
}

// One lane owns V adjacent environments for the whole trajectory. Per step it reads one action row, one saved state row and the
// cotangent rows that are present (a launch-uniform property: a loss on last_state alone reads none), and writes one gradient row
// per action row (the `substeps` contributions of a row are summed in registers). The loads of the next iteration are requested
// before the step's arithmetic, index clamped so that they are unconditional (DESIGN.md §4.1 "Pipeline"). Registers are
// component-major ([component][environment]): a 16-byte load lands in place.
// PGRAD: the static-parameter gradients pbv[P][V] stay in registers for the whole trajectory (like PMSM's omega_el cotangent) and
// leave after row 0, one coalesced [B] store per requested leaf; the batch sum is a launch of its own (param_sum.hip).
template <class M, typename T, int SOLVER, bool AHEAD, int V, bool PGRAD = false>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) sim_ahead_vjp_kernel(const VjpKernelArgs<T, M, PGRAD> ka) {
  constexpr int S = M::S, A = M::A, O = M::O;
  constexpr bool LEAN = vjp_lean_trig<T>();
  static_assert(!M::HAS_LUT, "no reverse mode for the saturated PMSM");
  // addresses are (uniform pointer + uniform element offset) + a 32-bit lane offset: the scalar base / vector offset form of the
  // global accesses — one offset register for all streams instead of a 64-bit address pair per stream and lane
  const int64_t blk0 = (int64_t)blockIdx.x * (BLOCK * V);  // first environment of the workgroup
  const unsigned lane0 = threadIdx.x * V;
  unsigned lane = lane0;  // refreshed per row (below): a loop-variant offset keeps the (pointer + lane) sums out of registers
  const int64_t i0 = blk0 + lane0;
  Ctx<T, M> c;
  load_ctx<false>(c, ka.kp, 0, ka.dt, ka.env_tau, ka.adv_coef);
  c.lin_stop = ka.lin_stop;
  c.lin_div = vjp_uniform(T(ka.K - 1));
  c.lin_last = ka.K - 1;
#pragma unroll
  for (int j = 0; j < S; ++j) c.nrm[j].y = vjp_uniform(c.nrm[j].y);
#pragma unroll
  for (int j = 0; j < (M::ND > 0 ? M::ND : 1); ++j) c.den[j].y = vjp_uniform(c.den[j].y);
  if (i0 >= ka.B) return;  // host: B % V == 0, a lane is whole or absent
  const int64_t B = ka.B, K = ka.K, N = ka.K * ka.substeps;
  const int64_t OW = O + ka.n_control;  // control columns are constants of the trajectory: their cotangent columns are skipped
  const int32_t sub_last = ka.substeps - 1;
  const bool has_gobs = ka.g_obs != nullptr;
  const bool dead = M::IS_PMSM ? (c.P[M::P - 1] > T(0)) : false;

  auto load_state_row = [&](int64_t n, T (&sv)[S][V]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j) load_v<T, V>((ka.straj[j] + (n * B + blk0)) + lane, sv[j]);
  };
  auto load_gobs_row = [&](int64_t n, T (&go)[O][V]) __attribute__((always_inline)) {
    if (has_gobs) {
#pragma unroll
      for (int q = 0; q < O; ++q) load_v<T, V>((ka.g_obs + ((n * OW + q) * B + blk0)) + lane, go[q]);
    }
  };
  auto load_gst_row = [&](int64_t n, T (&gs)[S][V]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j)
      if (ka.g_straj[j] != nullptr) load_v<T, V>((ka.g_straj[j] + (n * B + blk0)) + lane, gs[j]);
  };
  auto load_action = [&](int64_t k, T (&a)[A][V]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < A; ++q) load_v<T, V>((ka.actions + ((k * A + q) * B + blk0)) + lane, a[q]);
  };

  T sb[S][V];  // cotangent of the carried state
  T geps0[V], eps0[V];
#pragma unroll
  for (int v = 0; v < V; ++v) geps0[v] = eps0[v] = T(0);
  if constexpr (M::IS_PMSM && AHEAD) load_v<T, V>((ka.straj[2] + blk0) + lane, eps0);  // row 0: the wrapped initial angle (the clip is periodic in it)
  T om_c[V];  // PMSM: omega_el is a constant of the trajectory — row 0's value stands for every row's (same bits), no register per row
#pragma unroll
  for (int v = 0; v < V; ++v) om_c[v] = T(0);
  if constexpr (M::IS_PMSM) load_v<T, V>((ka.straj[6] + blk0) + lane, om_c);
  // PGRAD: gradient w.r.t. the static parameters, per environment: registers, or (vjp_pgrad_in_lds) the lane's own run of LDS
  constexpr bool PLDS = PGRAD && vjp_pgrad_in_lds<M, T, SOLVER>();
  constexpr int NPB = (PGRAD && !PLDS) ? M::P : 1;
  T pbv[NPB][V];
#pragma unroll
  for (int j = 0; j < NPB; ++j)
#pragma unroll
    for (int v = 0; v < V; ++v) pbv[j][v] = T(0);
  T* pbl = nullptr;
  if constexpr (PLDS) {
    static_assert(V == 1, "the LDS accumulators belong to one environment per lane");
    constexpr int PSTRIDE = M::P | 1;
    __shared__ T pbs[BLOCK * PSTRIDE];
    pbl = &pbs[threadIdx.x * PSTRIDE];
#pragma unroll
    for (int j = 0; j < M::P; ++j) pbl[j] = T(0);
  }

  // cotangent of a saved row -> cotangent of the carried state: r = observe^T gob + gst, through post^T where rows are post-processed
  auto add_row = [&](const T (&svh)[S][V], T (&r)[S], int v) __attribute__((always_inline)) {
    if constexpr (AHEAD) {
      T s1[S];
#pragma unroll
      for (int j = 0; j < S; ++j) s1[j] = svh[j][v];
      if constexpr (PLDS) {
        M::post_pvjp(s1, c, r, pbl);
      } else if constexpr (PGRAD && M::IS_PMSM) {  // the torque of the saved row reads l_d, l_q, psi_p
        T pl[M::P];
#pragma unroll
        for (int j = 0; j < M::P; ++j) pl[j] = pbv[j][v];
        M::post_pvjp(s1, c, r, pl);
#pragma unroll
        for (int j = 0; j < M::P; ++j) pbv[j][v] = pl[j];
      }
      M::post_vjp(s1, c, r);
      if constexpr (M::IS_PMSM) {  // the saved buffer columns: prev_clip with dead time, zeros without
        r[0] = dead ? r[0] : T(0);
        r[1] = dead ? r[1] : T(0);
      }
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (AHEAD && M::IS_PMSM && j == 5) continue;  // post_vjp has moved the torque's cotangent to the currents: stays exactly 0
      sb[j][v] = sb[j][v] + r[j];
    }
  };
  auto consume = [&](const T (&svh)[S][V], const T (&go)[O][V], const T (&gs)[S][V]) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      T r[S], s1[S];
#pragma unroll
      for (int j = 0; j < S; ++j) {
        r[j] = T(0);
        s1[j] = svh[j][v];
      }
      if (has_gobs) {
        T g[O];
#pragma unroll
        for (int q = 0; q < O; ++q) g[q] = go[q][v];
        M::template observe_vjp<LEAN>(s1, c, g, r);
      }
#pragma unroll
      for (int j = 0; j < S; ++j)
        if (ka.g_straj[j] != nullptr) r[j] = r[j] + gs[j][v];
      add_row(svh, r, v);
    }
  };

  T svh[S][V], svc[S][V], svn[S][V];  // saved rows n, n - 1 and (in flight) n - 2
  T go[O][V], gs[S][V];               // cotangent rows of row n
  T ah[A][V], ac[A][V], an[A][V];     // action rows k1 and k of step n - 1, k of step n - 2 (in flight)
  // last_state is row N: its cotangent first, on its own (with the cotangent rows of row N in flight next to it, the prologue
  // would be the kernel's register peak)
#pragma unroll
  for (int j = 0; j < S; ++j)
#pragma unroll
    for (int v = 0; v < V; ++v) sb[j][v] = T(0);
  load_state_row(N, svh);
  {
    T gl[S][V];
#pragma unroll
    for (int j = 0; j < S; ++j) {
#pragma unroll
      for (int v = 0; v < V; ++v) gl[j][v] = T(0);
      if (ka.g_last[j] != nullptr) load_v<T, V>((ka.g_last[j] + blk0) + lane, gl[j]);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      T r[S];
#pragma unroll
      for (int j = 0; j < S; ++j) r[j] = gl[j][v];
      add_row(svh, r, v);
    }
  }
  load_gobs_row(N, go);
  load_gst_row(N, gs);
  load_state_row(N > 0 ? N - 1 : 0, svc);
  if (N > 0) {
    load_action(K - 1, ah);
    load_action(K - 1, ac);
  }

  T acc[A][V];  // gradient of action row kacc, complete once the last step that read the row has been walked
#pragma unroll
  for (int q = 0; q < A; ++q)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[q][v] = T(0);
  auto store_acc = [&](int64_t row) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < A; ++q) store_stream<T, V>((ka.g_actions + ((row * A + q) * B + blk0)) + lane, acc[q]);
  };
  int64_t k = K - 1, kacc = K - 1;  // (k, sub): action row and sub-step of step n - 1
  int32_t sub = sub_last;
  for (int64_t n = N;; --n) {
    // the same value, but not a loop invariant to the optimiser: hoisted, every stream's (pointer + lane) would sit in a 64-bit
    // register pair for the whole trajectory; like this each access is scalar row base + this one 32-bit offset
    lane = (unsigned)__builtin_amdgcn_mov_dpp((int)lane0, 0xE4, 0xF, 0xF, false);
    consume(svh, go, gs);
    if (n == 0) break;
    // step n - 1 leads from row n - 1 to row n; what the next iteration reads is requested now
    int64_t kp = k;
    int32_t subp = sub - 1;
    if (subp < 0) {
      subp = sub_last;
      kp = (k > 0) ? k - 1 : 0;
    }
    constexpr bool LATE = vjp_late_cotangents<M, T, SOLVER, V>();
    constexpr bool LATE_ROW = LATE && M::IS_PMSM && sizeof(T) == 8;  // PMSM fp64 RK: the saved row and action row as well
    if constexpr (!LATE) {
      load_gobs_row(n - 1, go);
      load_gst_row(n - 1, gs);
    }
    if constexpr (!LATE_ROW) {
      load_state_row(n > 1 ? n - 2 : 0, svn);
      load_action(kp, an);
    }
    const int64_t k1 = (AHEAD && sub == sub_last && k < K - 1) ? k + 1 : k;  // the row of the c_i == 1 stages
    // rows: k1 == kacc always; k < kacc when this step is the last one that reads row kacc (wave-uniform): its own row's gradient
    // starts in accn, row kacc is complete with this step's c_i == 1 share and leaves
    const bool new_row = k != kacc;
    T accn[A][V];
    constexpr bool NO_C1 = SOLVER == EXCENV_EULER;  // no c_i == 1 stage: row kacc is complete before a step of another row
    if constexpr (NO_C1) {
      if (new_row) {
        store_acc(kacc);
#pragma unroll
        for (int q = 0; q < A; ++q)
#pragma unroll
          for (int v = 0; v < V; ++v) acc[q][v] = T(0);
      }
    }
    // PMSM's constants of the trajectory (initial angle, omega_el) in the forms that have no register to spare for them: read again
    // per row from row 0 (cache hits) instead of being held
    if constexpr (vjp_reload_constants<M, V>()) {
      if constexpr (AHEAD) load_v<T, V>((ka.straj[2] + blk0) + lane, eps0);
      load_v<T, V>((ka.straj[6] + blk0) + lane, om_c);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      T s0[S], s1[S], sbv[S], a0[A], a1[A], g0[A], g1[A];
#pragma unroll
      for (int j = 0; j < S; ++j) {
        s0[j] = svc[j][v];
        s1[j] = svh[j][v];
        sbv[j] = sb[j][v];
      }
      if constexpr (M::IS_PMSM) s0[6] = s1[6] = om_c[v];
#pragma unroll
      for (int q = 0; q < A; ++q) {
        a0[q] = ac[q][v];
        a1[q] = ah[q][v];
      }
      if constexpr (PLDS) {
        env_step_vjp<M, SOLVER, AHEAD, true>(s0, s1, a0, a1, k, k1, c, eps0[v], sbv, geps0[v], g0, g1, pbl);
      } else if constexpr (PGRAD) {
        T pl[M::P];
#pragma unroll
        for (int j = 0; j < M::P; ++j) pl[j] = pbv[j][v];
        env_step_vjp<M, SOLVER, AHEAD, true>(s0, s1, a0, a1, k, k1, c, eps0[v], sbv, geps0[v], g0, g1, pl);
#pragma unroll
        for (int j = 0; j < M::P; ++j) pbv[j][v] = pl[j];
      } else {
        env_step_vjp<M, SOLVER, AHEAD>(s0, s1, a0, a1, k, k1, c, eps0[v], sbv, geps0[v], g0, g1);
      }
#pragma unroll
      for (int j = 0; j < S; ++j) sb[j][v] = sbv[j];
#pragma unroll
      for (int q = 0; q < A; ++q) {
        if constexpr (NO_C1) {
          acc[q][v] = acc[q][v] + g0[q];
        } else if (k1 != k) {
          acc[q][v] = acc[q][v] + g1[q];
          accn[q][v] = g0[q];
        } else if (new_row) {
          accn[q][v] = g0[q] + g1[q];
        } else {
          acc[q][v] = acc[q][v] + (g0[q] + g1[q]);
        }
      }
    }
    if constexpr (!NO_C1) {
      if (new_row) store_acc(kacc);
    }
    // (behind the store: nothing can be moved in front of it)
    if constexpr (LATE_ROW) {
      load_state_row(n > 1 ? n - 2 : 0, svn);
      load_action(kp, an);
    }
    if constexpr (LATE) {
      load_gobs_row(n - 1, go);
      load_gst_row(n - 1, gs);
    }
    if constexpr (!NO_C1) {
      if (new_row) {
#pragma unroll
        for (int q = 0; q < A; ++q)
#pragma unroll
          for (int v = 0; v < V; ++v) acc[q][v] = accn[q][v];
      }
    }
    kacc = k;
#pragma unroll
    for (int j = 0; j < S; ++j)
#pragma unroll
      for (int v = 0; v < V; ++v) {
        svh[j][v] = svc[j][v];
        svc[j][v] = svn[j][v];
      }
#pragma unroll
    for (int q = 0; q < A; ++q)
#pragma unroll
      for (int v = 0; v < V; ++v) {
        ah[q][v] = ac[q][v];
        ac[q][v] = an[q][v];
      }
    k = kp;
    sub = subp;
  }
  if (N > 0) store_acc(kacc);
  if constexpr (M::IS_PMSM && AHEAD) {
#pragma unroll
    for (int v = 0; v < V; ++v) sb[2][v] = sb[2][v] + geps0[v];
  }
#pragma unroll
  for (int j = 0; j < S; ++j) store_v<T, V>((ka.g_state_in[j] + blk0) + lane, sb[j]);
  if constexpr (PGRAD) {
#pragma unroll
    for (int j = 0; j < M::P; ++j) {
      if (ka.g_params[j] == nullptr) continue;
      if constexpr (PLDS) {
        const T one[1] = {pbl[j]};
        store_v<T, 1>((ka.g_params[j] + blk0) + lane, one);
      } else {
        store_v<T, V>((ka.g_params[j] + blk0) + lane, pbv[j]);
      }
    }
  }
}

// The raw levels of the tank under EXCENV_SEM_AHEAD (vjp.hpp vjp_needs_raw_rows): the forward's own steps (env_advance_raw) again,
// one environment per lane, from the saved rows into raw[N + 1][B]. A saved row above 0 IS the raw level (the clamp is the identity
// there) and restarts the recurrence; a saved 0 stands for a raw level at or below 0, which the recurrence carries on from the last
// wet row. Row 0 is taken as saved: an initial level below 0 — outside the model's range — is read as 0. One pass of the forward's
// arithmetic without its stores of observations: cheaper than the forward launch it follows.
template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(BLOCK) vjp_raw_rows_kernel(const VjpArgs<T, M> ka, T* __restrict__ raw) {
  static_assert(M::S == 1 && M::A == 1 && !M::IS_PMSM, "the tank: one level, one action");
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  Ctx<T, M> c;
  load_ctx<false>(c, ka.kp, 0, ka.dt, ka.env_tau, ka.adv_coef);
  if (i >= ka.B) return;
  const int64_t B = ka.B, K = ka.K, N = ka.K * ka.substeps;
  AheadAux<T> aux{};
  T st[1] = {ka.straj[0][i]};
  int64_t k = 0;
  int32_t sub = 0;
  for (int64_t n = 0;; ++n) {
    const T saved = ka.straj[0][n * B + i];
    st[0] = (saved > T(0)) ? saved : st[0];
    raw[n * B + i] = st[0];
    if (n == N) break;
    const bool last_sub = sub == ka.substeps - 1;
    const int64_t k1 = (last_sub && k < K - 1) ? k + 1 : k;  // the row of the c_i == 1 stages
    const T a[1] = {ka.actions[k * B + i]}, a1[1] = {ka.actions[k1 * B + i]};
    env_advance_raw<M, SOLVER>(st, a, a1, k, k1, c, aux);
    sub = last_sub ? 0 : sub + 1;
    k = last_sub ? k + 1 : k;
  }
}

// Packs VjpArgs and launches the instantiation the call names (vjp.hpp vjp_instantiated): every other combination is an error
template <class M, typename T> static int launch_vjp(const VjpCall& vc) {
  VjpParamArgs<T, M> ka;  // the plain launch passes its VjpArgs part
  std::memset(&ka, 0, sizeof(ka));
  const bool ahead = vc.semantics == EXCENV_SEM_AHEAD;
  if (int rc = reverse_preamble("excenv_sim_ahead_vjp", ka, vc.props, vc.obs_stepsize, vc.env_tau, ahead)) return rc;
  if (int rc = pmsm_one_substep<M>(vc.substeps)) return rc;
  ka.B = vc.B;
  ka.K = vc.K;
  ka.substeps = vc.substeps;
  ka.n_control = vc.n_control;
  ka.actions = (const T*)vc.actions;
  ka.g_obs = (const T*)vc.grad_obs_traj;
  ka.g_actions = (T*)vc.grad_actions;
  for (int j = 0; j < M::S; ++j) {
    if (!vc.state_traj[j] || !vc.grad_state_in[j]) { set_error("excenv_sim_ahead_vjp: state pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.straj[j] = (const T*)vc.state_traj[j];
    ka.g_straj[j] = vc.grad_state_traj ? (const T*)vc.grad_state_traj[j] : nullptr;
    ka.g_last[j] = vc.grad_last_state ? (const T*)vc.grad_last_state[j] : nullptr;
    ka.g_state_in[j] = (T*)vc.grad_state_in[j];
  }
  ka.lin_stop = (T)(vc.env_tau * (double)(vc.K > 0 ? vc.K - 1 : 0));
  const bool pgrad = vc.grad_params != nullptr;
  for (int j = 0; pgrad && j < M::P; ++j) ka.g_params[j] = (T*)vc.grad_params[j];
  if (vc.B == 0) return EXCENV_OK;
  const dim3 grid((unsigned)((vc.B / vc.V + BLOCK - 1) / BLOCK)), block(BLOCK);
  const hipStream_t stream = (hipStream_t)vc.stream;
  if constexpr (M::ID == EXCENV_FLUID_TANK) {
    if (vc.raw_rows != nullptr) {  // the reverse kernel reads the raw levels in place of the saved (clamped) ones
      const dim3 grid1((unsigned)((vc.B + BLOCK - 1) / BLOCK));
      if (vc.solver == EXCENV_RK4) hipLaunchKernelGGL((vjp_raw_rows_kernel<M, T, EXCENV_RK4>), grid1, block, 0, stream, ka, (T*)vc.raw_rows);
      else hipLaunchKernelGGL((vjp_raw_rows_kernel<M, T, EXCENV_TSIT5>), grid1, block, 0, stream, ka, (T*)vc.raw_rows);
      if (int rc = check_launch("excenv_sim_ahead_vjp (raw rows)")) return rc;
      ka.straj[0] = (const T*)vc.raw_rows;
    }
  }
  const bool launched = vjp_instantiated(vc.semantics, M::ID, (int)sizeof(T), vc.solver, M::HAS_LUT, vc.V, pgrad) && with_solver(vc.solver, [&](auto solver) {
    return with_flag(ahead, [&](auto ah) {
      return with_const<1, 2, 4>(vc.V, [&](auto v) {
        return with_flag(pgrad, [&](auto pg) {
          constexpr int SOLVER = decltype(solver)::value, VV = decltype(v)::value;
          constexpr bool AH = decltype(ah)::value, PG = decltype(pg)::value;
          if constexpr (!vjp_instantiated(AH ? EXCENV_SEM_AHEAD : EXCENV_SEM_STEP, M::ID, (int)sizeof(T), SOLVER, M::HAS_LUT, VV, PG)) {
            return false;
          } else {
            const VjpKernelArgs<T, M, PG>& kk = ka;
            hipLaunchKernelGGL((sim_ahead_vjp_kernel<M, T, SOLVER, AH, VV, PG>), grid, block, 0, stream, kk);
            return true;
          }
        });
      });
    });
  });
  if (!launched) {
    set_error("excenv_sim_ahead_vjp: no kernel instantiation (semantics %d, %d-byte elements, V=%d)", vc.semantics, (int)sizeof(T), vc.V);
    return EXCENV_EINVAL;
  }
  g_last_launch = vjp_name(vc.V, pgrad);
  return check_launch("excenv_sim_ahead_vjp");
}

// EnvVTable::sim_vjp (launch.hpp): a model's translation unit vjp_<model>.hip instantiates it
template <template <typename> class MT> int vjp_entry(const VjpCall& vc) {
  if constexpr (MT<float>::HAS_LUT) {
    set_error("excenv_sim_ahead_vjp: the saturated PMSM (pmsm_lut) has no reverse mode");
    return EXCENV_EUNSUPPORTED;
  } else {
    return EXCENV_BY_DTYPE(launch_vjp, MT, vc);
  }
}

}  // namespace excenv
