// Linearisation of the step kernel: one launch writes the Jacobians d x+ / d x and d x+ / d a (or those of the observation) of `rows`
// stored steps of B environments. Shaped like step_vjp_kernel (kernels_step_vjp.hpp): one lane per step instance
// (trajectory row n, environment i), the two saved states and the action held in registers; the Jacobian leaves row by row, each row
// one reverse sweep of the step from a one-hot cotangent. The arithmetic is step_vjp_kernel's own (env_step_vjp<M, SOLVER,
// /*AHEAD=*/false> of kernels_vjp.hpp and the transposed functions of models.hpp), so row r is bit for bit what that kernel returns
// for the cotangent e_r wherever the compiler schedules both alike. No LDS, no inline assembly, no scratch.
// Instantiated in step_jac_<model>.hip only.
#pragma once
#include "kernels_vjp.hpp"
#include "step_jac.hpp"

namespace excenv {

template <typename T, class M> struct StepJacArgs {
  KProps<T, M> kp;
  int64_t B, rows;
  uint32_t blocks_per_row;                     // workgroups of one trajectory row: a workgroup never spans two rows
  int32_t substeps;                            // steps per action row
  int32_t obs_rows;                            // 0: rows of the new state, 1: rows of its observation
  int64_t s_row;                               // elements between two trajectory rows of a state leaf
  const T* state_in[M::S];                     // step n starts at state_in[j][n * s_row + i]
  const T* state_out[M::S];                    // and ends at state_out[j][n * s_row + i], the post-processed state the forward saved
  const T* action;                             // (row k, component q, environment i) at k * a_row + q * a_comp + i * a_env
  int64_t a_row, a_comp, a_env;
  T* jac;                                      // [rows][R][S + A][B]
  T dt, env_tau, adv_coef;
};

// One lane per step instance. The lane reads the step's two states and its action once, then walks the R rows of the Jacobian at
// run time: the cotangent of row r is e_r on the new state (or observe^T e_r at the saved new state), it goes through the transposed
// step exactly as in step_vjp_kernel, and the S + A entries of the row leave as one coalesced [B] piece per column. The loop is not
// unrolled: its body is a whole RK adjoint. A lane past the batch end reads and writes nothing.
template <class M, typename T, int SOLVER>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) step_jac_kernel(const StepJacArgs<T, M> ka) {
  constexpr int S = M::S, A = M::A, O = M::O;
  constexpr bool LEAN = vjp_lean_trig<T>();
  static_assert(!M::HAS_LUT, "no reverse mode for the saturated PMSM");
  const int64_t n = blockIdx.x / ka.blocks_per_row;  // wave-uniform
  const int64_t i = (int64_t)(blockIdx.x % ka.blocks_per_row) * BLOCK + threadIdx.x;
  Ctx<T, M> c;
  load_ctx<false>(c, ka.kp, 0, ka.dt, ka.env_tau, ka.adv_coef);
  c.lin_stop = T(0);  // the trajectory clock of EXCENV_SEM_AHEAD: not read by a step
  c.lin_div = T(1);
  c.lin_last = 0;
#pragma unroll
  for (int j = 0; j < S; ++j) c.nrm[j].y = vjp_uniform(c.nrm[j].y);
#pragma unroll
  for (int j = 0; j < (M::ND > 0 ? M::ND : 1); ++j) c.den[j].y = vjp_uniform(c.den[j].y);
  if (i >= ka.B || n >= ka.rows) return;

  T s0[S], s1[S], a[A];
  const int64_t srow = n * ka.s_row + i;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    s0[j] = ka.state_in[j][srow];
    s1[j] = ka.state_out[j][srow];
  }
  const T* arow = ka.action + ((n / ka.substeps) * ka.a_row + i * ka.a_env);
#pragma unroll
  for (int q = 0; q < A; ++q) a[q] = arow[q * ka.a_comp];

  const bool obs_rows = ka.obs_rows != 0;
  const int R = obs_rows ? O : S;
  T* out = ka.jac + (n * R * (S + A) * ka.B + i);
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    T sb[S];
#pragma unroll
    for (int j = 0; j < S; ++j) sb[j] = T(0);
    if (obs_rows) {
      T g[O];
#pragma unroll
      for (int q = 0; q < O; ++q) g[q] = (q == r) ? T(1) : T(0);
      M::template observe_vjp<LEAN>(s1, c, g, sb);
    } else {
#pragma unroll
      for (int j = 0; j < S; ++j) sb[j] = (j == r) ? T(1) : T(0);
    }
    // s0 and a are the same for every row, and the compiler hoists what it can of the forward stage slopes out of the loop: welcome
    // while the registers are there (at most 217 are used). Should an instantiation leave the budget, start the step from
    // vjp_opaque copies of s0 and a here (kernels_vjp.hpp "the register budget"); tests/test_linearize_host.py checks the budget.
    T geps0 = T(0), gk[A], gk1[A];
    env_step_vjp<M, SOLVER, false>(s0, s1, a, a, 0, 0, c, T(0), sb, geps0, gk, gk1);
#pragma unroll
    for (int j = 0; j < S; ++j) out[j * ka.B] = sb[j];
#pragma unroll
    for (int q = 0; q < A; ++q) out[(S + q) * ka.B] = (SOLVER == EXCENV_EULER) ? gk[q] : gk[q] + gk1[q];  // the c_i == 1 stages read the same row
    out += (S + A) * ka.B;
  }
}

// Packs StepJacArgs and launches the instantiation the call names
template <class M, typename T> static int launch_step_jac(const StepJacCall& jc) {
  StepJacArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  if (int rc = reverse_preamble("excenv_step_jacobian", ka, jc.props, jc.dt, jc.env_tau, false)) return rc;
  if (int rc = pmsm_one_substep<M>(jc.substeps)) return rc;
  ka.B = jc.B;
  ka.rows = jc.rows;
  ka.substeps = jc.substeps;
  ka.obs_rows = jc.row_kind == EXCENV_JAC_OBS;
  ka.s_row = jc.state_row_stride;
  for (int j = 0; j < M::S; ++j) {
    ka.state_in[j] = (const T*)jc.state_in[j];
    ka.state_out[j] = (const T*)jc.state_out[j];
  }
  ka.action = (const T*)jc.action;
  ka.a_row = jc.a_row;
  ka.a_comp = jc.a_comp;
  ka.a_env = jc.a_env;
  ka.jac = (T*)jc.jacobian;
  if (jc.B == 0 || jc.rows == 0) return EXCENV_OK;
  const int64_t per_row = (jc.B + BLOCK - 1) / BLOCK;
  if (per_row * jc.rows > (int64_t)0x7fffffff) {
    set_error("excenv_step_jacobian: rows * ceil(B / %d) = %lld workgroups exceed one launch", BLOCK, (long long)(per_row * jc.rows));
    return EXCENV_EINVAL;
  }
  ka.blocks_per_row = (uint32_t)per_row;
  const dim3 grid((unsigned)(per_row * jc.rows)), block(BLOCK);
  const hipStream_t stream = (hipStream_t)jc.stream;
  const bool launched = jc.V == 1 && with_solver(jc.solver, [&](auto solver) {
    hipLaunchKernelGGL((step_jac_kernel<M, T, decltype(solver)::value>), grid, block, 0, stream, ka);
    return true;
  });
  if (!launched) {
    set_error("excenv_step_jacobian: no kernel instantiation (%d-byte elements, V=%d)", (int)sizeof(T), jc.V);
    return EXCENV_EINVAL;
  }
  g_last_launch = step_jac_name(jc.row_kind);
  return check_launch("excenv_step_jacobian");
}

// EnvVTable::step_jac (launch.hpp): a model's translation unit step_jac_<model>.hip instantiates it
template <template <typename> class MT> int step_jac_entry(const StepJacCall& jc) {
  if constexpr (MT<float>::HAS_LUT) {
    set_error("excenv_step_jacobian: the saturated PMSM (pmsm_lut) has no reverse mode");
    return EXCENV_EUNSUPPORTED;
  } else {
    return EXCENV_BY_DTYPE(launch_step_jac, MT, jc);
  }
}

}  // namespace excenv
