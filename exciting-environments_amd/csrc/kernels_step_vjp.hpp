// Reverse mode of the step kernel: one launch computes the vector-Jacobian product of ONE excenv_step / excenv_gym_step call from
// the two states of that call (DESIGN.md §4.9 "Step"). Shaped like step_kernel (kernels.hpp), not like the trajectory kernel: one lane
// per environment, [B] state leaves, row-major action and observation-cotangent rows; the arithmetic is the trajectory kernel's own
// (env_step_vjp<M, SOLVER, /*AHEAD=*/false> of kernels_vjp.hpp and the transposed functions of models.hpp), with the reward's
// transpose (env_reward_vjp) folded into the same launch. No LDS, no inline assembly, no scratch.
// Instantiated in step_vjp_<model>.hip only.
#pragma once
#include "kernels_vjp.hpp"
#include "step_vjp.hpp"

namespace excenv {

template <typename T, class M> struct StepVjpArgs {
  KProps<T, M> kp;
  int64_t B;
  int32_t n_control;                           // the observation cotangent has O + n_control columns
  int32_t control_idx[EXCENV_MAX_CONTROL];     // read with a reward cotangent only
  const T* reference[EXCENV_MAX_CONTROL];      // [B] each, likewise
  const T* state_in[M::S];                     // [B]
  const T* state_out[M::S];                    // [B]: the post-processed row the forward returned
  const T* action;                             // [B][A]
  const T* g_obs;                              // [B][O + n_control] or nullptr
  const T* g_state_out[M::S];                  // [B] or nullptr, per leaf
  const T* g_reward;                           // [B] or nullptr
  T* g_state_in[M::S];                         // [B]
  T* g_action;                                 // [B][A]
  T dt, env_tau, adv_coef;
};

// One lane per environment (V == 1, the only form): reads the step's two states, its action row and the cotangents that are present
// (each group is a launch-uniform property: an absent one loads nothing), and writes the gradients of the starting state and of the
// action row. The carried cotangent starts as
//   r = observe^T grad_obs + grad_state_out + reward^T grad_reward      (all at the saved, post-processed state_out)
// and goes through the transposed step exactly as a row of the trajectory kernel under EXCENV_SEM_STEP does. Control columns of
// grad_obs are skipped: references get no gradient. A lane past the batch end reads and writes nothing.
template <class M, typename T, int SOLVER, int V>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) step_vjp_kernel(const StepVjpArgs<T, M> ka) {
  constexpr int S = M::S, A = M::A, O = M::O;
  constexpr bool LEAN = vjp_lean_trig<T>();
  static_assert(!M::HAS_LUT, "no reverse mode for the saturated PMSM");
  static_assert(V == 1, "one environment per lane");
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  Ctx<T, M> c;
  load_ctx<false>(c, ka.kp, 0, ka.dt, ka.env_tau, ka.adv_coef);
  c.lin_stop = T(0);  // the trajectory clock of EXCENV_SEM_AHEAD: not read by a step
  c.lin_div = T(1);
  c.lin_last = 0;
#pragma unroll
  for (int j = 0; j < S; ++j) c.nrm[j].y = vjp_uniform(c.nrm[j].y);
#pragma unroll
  for (int j = 0; j < (M::ND > 0 ? M::ND : 1); ++j) c.den[j].y = vjp_uniform(c.den[j].y);
  if (i >= ka.B) return;

  T s0[S], s1[S], sb[S], a[A];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    s0[j] = ka.state_in[j][i];
    s1[j] = ka.state_out[j][i];
    sb[j] = T(0);
  }
  load_row<T, A>(ka.action + i * A, a);
  if (ka.g_obs != nullptr) {
    T g[O];
    if (ka.n_control == 0) {
      load_row<T, O>(ka.g_obs + i * O, g);
    } else {
      const T* row = ka.g_obs + i * (O + ka.n_control);
#pragma unroll
      for (int q = 0; q < O; ++q) g[q] = row[q];
    }
    M::template observe_vjp<LEAN>(s1, c, g, sb);
  }
#pragma unroll
  for (int j = 0; j < S; ++j)
    if (ka.g_state_out[j] != nullptr) sb[j] = sb[j] + ka.g_state_out[j][i];
  if (ka.g_reward != nullptr) {
    T rref[EXCENV_MAX_CONTROL];
#pragma unroll
    for (int j = 0; j < EXCENV_MAX_CONTROL; ++j) rref[j] = (j < ka.n_control) ? ka.reference[j][i] : T(0);
    env_reward_vjp<M, T>(s1, c, ka.n_control, ka.control_idx, rref, ka.g_reward[i], sb);
  }

  T geps0 = T(0), gk[A], gk1[A], ga[A];
  env_step_vjp<M, SOLVER, false>(s0, s1, a, a, 0, 0, c, T(0), sb, geps0, gk, gk1);
#pragma unroll
  for (int q = 0; q < A; ++q) ga[q] = (SOLVER == EXCENV_EULER) ? gk[q] : gk[q] + gk1[q];  // the c_i == 1 stages read the same row
  store_row<T, A>(ka.g_action + i * A, ga);
#pragma unroll
  for (int j = 0; j < S; ++j) ka.g_state_in[j][i] = sb[j];
}

// Packs StepVjpArgs and launches the instantiation the call names
template <class M, typename T> static int launch_step_vjp(const StepVjpCall& sc) {
  StepVjpArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  if (int rc = reverse_preamble("excenv_step_vjp", ka, sc.props, sc.tau, sc.tau, false)) return rc;
  ka.B = sc.B;
  ka.n_control = sc.control ? sc.control->n_control : 0;
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = sc.control->control_idx[j];
    ka.reference[j] = (const T*)sc.control->reference[j];
  }
  for (int j = 0; j < M::S; ++j) {
    ka.state_in[j] = (const T*)sc.state_in[j];
    ka.state_out[j] = (const T*)sc.state_out[j];
    ka.g_state_out[j] = sc.grad_state_out ? (const T*)sc.grad_state_out[j] : nullptr;
    ka.g_state_in[j] = (T*)sc.grad_state_in[j];
  }
  ka.action = (const T*)sc.action;
  ka.g_obs = (const T*)sc.grad_obs;
  ka.g_reward = (const T*)sc.grad_reward;
  ka.g_action = (T*)sc.grad_action;
  if (sc.B == 0) return EXCENV_OK;
  const dim3 grid((unsigned)((sc.B + BLOCK - 1) / BLOCK)), block(BLOCK);
  const hipStream_t stream = (hipStream_t)sc.stream;
  const bool launched = sc.V == 1 && with_solver(sc.solver, [&](auto solver) {
    hipLaunchKernelGGL((step_vjp_kernel<M, T, decltype(solver)::value, 1>), grid, block, 0, stream, ka);
    return true;
  });
  if (!launched) {
    set_error("excenv_step_vjp: no kernel instantiation (%d-byte elements, V=%d)", (int)sizeof(T), sc.V);
    return EXCENV_EINVAL;
  }
  g_last_launch = step_vjp_name(sc.V);
  return check_launch("excenv_step_vjp");
}

// EnvVTable::step_vjp (launch.hpp): a model's translation unit step_vjp_<model>.hip instantiates it
template <template <typename> class MT> int step_vjp_entry(const StepVjpCall& sc) {
  if constexpr (MT<float>::HAS_LUT) {
    set_error("excenv_step_vjp: the saturated PMSM (pmsm_lut) has no reverse mode");
    return EXCENV_EUNSUPPORTED;
  } else {
    return EXCENV_BY_DTYPE(launch_step_vjp, MT, sc);
  }
}

}  // namespace excenv
