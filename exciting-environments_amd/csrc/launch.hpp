// Host-side glue between the C ABI (include/excenv.h) and the templated kernels: converts the untyped
// call into typed kernel arguments, picks the instantiation, enqueues it on the caller's stream.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include "kernels_emr.hpp"
#include "feedback.hpp"
#include "feedback_vjp.hpp"
#include "policy.hpp"
#include "refgen.hpp"
#include "rew_vjp.hpp"
#include "step_jac.hpp"
#include "step_vjp.hpp"
#include "vjp.hpp"

namespace excenv {

void set_error(const char* fmt, ...);
// Set by launch_dyn when raising a kernel's dynamic-LDS limit failed (the launch is then skipped and
// check_launch reports the stored message instead of a generic launch error). Per thread, like the error string.
static thread_local bool g_attr_failed = false;
// Which kernel form the last launching call of this thread enqueued: excenv_sim_ahead[_ws], excenv_step and the reverse-mode calls
// (excenv_last_launch(): tests assert that the path they mean to check is the one that ran; like the error string it is per thread
// and purely informational).
extern thread_local const char* g_last_launch;  // defined in excenv_api.hip

struct StepCall {
  int vec_pref;  // 0 auto, else forced envs per lane
  int solver, dtype;
  int64_t B;
  const excenv_props_t* props;
  const excenv_control_t* control;  // nullptr when n_control == 0
  double tau;
  const void* const* state_in;
  const void* action;
  void* const* state_out;
  void* obs;
  void* reward;       // optional gym outputs
  void* terminated;
  void* truncated;
  hipStream_t stream;
};

struct SimCall {
  int solver, dtype;
  int64_t B, K;
  int32_t substeps;
  const excenv_props_t* props;
  const excenv_control_t* control;
  double obs_stepsize, env_tau;
  const void* const* state_in;
  const void* actions;
  int action_layout;
  void* obs_traj;
  void* const* state_traj;  // may be nullptr
  int traj_layout;
  void* const* last_state;
  int semantics;
  int lds_pad;   // dynamic LDS bytes per workgroup (occupancy shaping experiments; 0 = none)
  const excenv_traj_gym_t* gym;  // optional reward / terminated / truncated trajectories
  hipStream_t stream;
  SimPlan plan;  // sim_plan(): the form of the trajectory kernel
  bool keep_const = false;  // EXCENV_OPT_KEEP_CONSTANT_COLUMNS on the caller's own lane-major trajectory buffers
};

struct TrajGymCall {
  int dtype;
  int64_t B, rows;
  const excenv_props_t* props;
  const excenv_control_t* control;
  const int64_t* ref_strides;  // [n_control][2] element strides (env, row) of each reference array
  const void* const* state_traj;
  int64_t s_sb, s_sk;  // element strides (env, row) of every state leaf
  void* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  int out_layout;
  hipStream_t stream;
};

struct FromObsCall {
  int dtype;
  int64_t B;
  const excenv_props_t* props;
  int32_t n_control;
  const int32_t* control_idx;
  const void* obs;
  void* const* state_out;
  void* const* reference_out;
  hipStream_t stream;
};

struct ObserveCall {
  int dtype;
  int64_t B;
  const excenv_props_t* props;
  const excenv_control_t* control;
  const void* const* state;
  void* obs;
  hipStream_t stream;
};

struct RefGenCall {
  int dtype;
  int64_t B;
  const excenv_props_t* props;
  int32_t n_control;
  const int32_t* control_idx;
  void* const* reference;
  int64_t* keys;
  int64_t* hold;
  int32_t hold_min, hold_max;
  hipStream_t stream;
  // inputs of the out-of-place form (nullptr: in place)
  const void* const* reference_in = nullptr;
  const int64_t* keys_in = nullptr;
  const int64_t* hold_in = nullptr;
};

struct RandomStateCall {
  int dtype;
  int64_t B;
  const excenv_props_t* props;
  const int64_t* keys;
  void* const* state_out;
  int64_t* key_leaf;
  hipStream_t stream;
};

struct EnvVTable {
  int S, A, O, P;
  int (*step)(const StepCall&);
  int (*sim)(const SimCall&);
  int (*traj_gym)(const TrajGymCall&);
  int (*from_obs)(const FromObsCall&);
  int (*update_ref)(const RefGenCall&);
  int (*random_state)(const RandomStateCall&);
  int (*observe)(const ObserveCall&);
  int (*sim_vjp)(const VjpCall&);  // reverse mode of sim (kernels_vjp.hpp)
  int (*rew_vjp)(const RewVjpCall&);  // reverse mode of traj_gym's reward (kernels_rew_vjp.hpp)
  int (*step_vjp)(const StepVjpCall&);  // reverse mode of step (kernels_step_vjp.hpp)
  int (*step_jac)(const StepJacCall&);  // Jacobians of step, row by row (kernels_step_jac.hpp)
  int (*sim_feedback)(const FeedbackCall&);  // sim with the actions computed in the launch (kernels_feedback.hpp)
  int (*sim_feedback_vjp)(const FeedbackVjpCall&);  // reverse mode of sim_feedback (kernels_feedback_vjp.hpp)
  int (*sim_policy)(const PolicyCall&);  // sim with the actions computed by an MLP in the launch (kernels_policy.hpp)
  int (*sim_policy_episodes)(const EpisodeCall&);  // sim_policy with gym outputs and resets in the launch (kernels_policy_episodes.hpp)
  int (*sim_policy_vjp)(const PolicyVjpCall&);  // reverse mode of sim_policy (kernels_policy_vjp.hpp)
};

// The reverse-mode entries of a model and its closed-loop entry: declared here so that they sit in the same table as every other entry
// point, each defined next to its launcher (kernels_vjp.hpp, kernels_rew_vjp.hpp, kernels_step_vjp.hpp, kernels_step_jac.hpp,
// kernels_feedback.hpp, kernels_feedback_vjp.hpp) and instantiated in the translation units that hold its kernels: vjp_<model>.hip,
// rew_vjp.hip, step_vjp_<model>.hip, step_jac_<model>.hip, feedback_<model>.hip, feedback_vjp_<model>.hip
template <template <typename> class MT> int vjp_entry(const VjpCall&);
template <template <typename> class MT> int rew_vjp_entry(const RewVjpCall&);
template <template <typename> class MT> int step_vjp_entry(const StepVjpCall&);
template <template <typename> class MT> int step_jac_entry(const StepJacCall&);
template <template <typename> class MT> int feedback_entry(const FeedbackCall&);
template <template <typename> class MT> int feedback_vjp_entry(const FeedbackVjpCall&);
template <template <typename> class MT> int policy_entry(const PolicyCall&);  // kernels_policy.hpp, policy_<model>.hip
template <template <typename> class MT> int policy_episodes_entry(const EpisodeCall&);  // kernels_policy_episodes.hpp, policy_episodes_<model>.hip
template <template <typename> class MT> int policy_vjp_entry(const PolicyVjpCall&);  // kernels_policy_vjp.hpp, policy_vjp_<model>.hip

// The one choice of the element type: launcher<MT<float>, float>(call) or launcher<MT<double>, double>(call) by the call's dtype
#define EXCENV_BY_DTYPE(launcher, MT, call) \
  ((call).dtype == EXCENV_F32 ? launcher<MT<float>, float>(call) : launcher<MT<double>, double>(call))

template <typename T, class M>
static bool fill_props(KProps<T, M>& kp, const excenv_props_t* p) {
  bool batched = false;
  int n = 0;
  auto put = [&](const excenv_param_t& q) {
    kp.scalar[n] = (T)q.value;
    kp.ptr[n] = (const T*)q.per_env;
    batched |= (q.per_env != nullptr);
    ++n;
  };
  for (int j = 0; j < M::P; ++j) put(p->static_params[j]);
  for (int j = 0; j < M::S; ++j) put(p->state_min[j]);
  for (int j = 0; j < M::S; ++j) put(p->state_max[j]);
  for (int j = 0; j < M::A; ++j) put(p->action_min[j]);
  for (int j = 0; j < M::A; ++j) put(p->action_max[j]);
  kp.lut_gd = kp.lut_gq = kp.lut_tab = nullptr;
  kp.lut_nd = kp.lut_nq = 0;
  kp.lut_lds = 0;
  if (p->pmsm_lut) {
    kp.lut_gd = (const T*)p->pmsm_lut->grid_d;
    kp.lut_gq = (const T*)p->pmsm_lut->grid_q;
    kp.lut_tab = (const T*)p->pmsm_lut->tables;
    kp.lut_nd = p->pmsm_lut->n_d;
    kp.lut_nq = p->pmsm_lut->n_q;
  }
  return batched;
}

// Launch with dynamic LDS; above the default 64 KiB limit the kernel's attribute is raised first (gfx950: 160 KiB per CU).
template <typename... P, typename... A>
static void launch_dyn(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d) failed: %s", (int)lds, hipGetErrorString(e));
      g_attr_failed = true;
      return;
    }
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

// A run-time value as a template argument: f(std::integral_constant<int, I>{}) for the I of the list that equals v. Returns what f
// returns (whether it launched), false when no I matches.
template <int... I, class F> static bool with_const(int v, F&& f) { return ((v == I && f(std::integral_constant<int, I>{})) || ...); }
template <class F> static bool with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// The call's solver (check_common has validated the id)
template <class F> static bool with_solver(int solver, F&& f) {
  return with_const<EXCENV_EULER, EXCENV_RK4, EXCENV_TSIT5>(solver, static_cast<F&&>(f));
}

// Dynamic LDS for the saturated model's tables: staged when they fit LDS (<= 150 KiB, leaving room for one workgroup).
// `other`: further dynamic LDS of the launch (returned with the tables' share); `static_bytes`: static LDS of the kernel itself
// (step_kernel's dense observation staging) — it counts against the workgroup's limit but is not part of the dynamic size.
template <typename T, class M> static size_t lut_lds_bytes(KProps<T, M>& kp, size_t other, size_t static_bytes = 0) {
  if constexpr (!M::HAS_LUT) return other;
  const size_t need = ((size_t)kp.lut_nd * kp.lut_nq * 8 + 2 * (size_t)(kp.lut_nd + kp.lut_nq)) * sizeof(T);  // tables, grids, cell-width reciprocals
  if (kp.lut_tab && need + other + static_bytes <= 150 * 1024) {
    kp.lut_lds = 1;
    return need + other;
  }
  kp.lut_lds = 0;
  return other;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int check_launch(const char* what) {
  if (g_attr_failed) {  // message already set by launch_dyn
    g_attr_failed = false;
    (void)hipGetLastError();
    return EXCENV_EHIP;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
    return EXCENV_EHIP;
  }
  return EXCENV_OK;
}

// PMSM dead time: a broadcast non-negative integer. The reference's state holds ONE buffered action, so any deadtime > 0 is a
// one-step delay (PMSM.step, pmsm_env.py:866-875) while the clip's angle advance uses the full (deadtime + 0.5) * tau
// (pmsm_env.py:599-604) — returned here, folded in double like the Python expression. `ahead`: the reference's sim_ahead
// override assembles deadtime + K buffer rows for K + 1 saved rows (pmsm_env.py:765-791), which only works for deadtime 0 / 1
// (its own vmap rejects the shapes otherwise), so EXCENV_SEM_AHEAD takes 0 / 1 only; EXCENV_SEM_STEP (K exact steps) takes any.
template <class M> static int pmsm_coef(const excenv_props_t* p, double env_tau, double* coef, bool ahead = false) {
  *coef = 0.0;
  if constexpr (M::IS_PMSM) {
    const excenv_param_t& d = p->static_params[6];
    if (d.per_env) {
      set_error("PMSM: static_params.deadtime must be a scalar, not a per-env array");
      return EXCENV_EUNSUPPORTED;
    }
    if (!(d.value >= 0.0) || d.value != (double)(int64_t)d.value || d.value > 1e6) {
      set_error("PMSM: deadtime must be a non-negative integer (got %g)", d.value);
      return EXCENV_EUNSUPPORTED;
    }
    if (ahead && d.value > 1.0) {
      set_error("PMSM: EXCENV_SEM_AHEAD supports deadtime 0 or 1 (got %g): the reference's sim_ahead builds K + deadtime buffer "
                "rows for K + 1 saved rows (pmsm_env.py:765-791) and fails for more; use EXCENV_SEM_STEP", d.value);
      return EXCENV_EUNSUPPORTED;
    }
    *coef = (d.value + 0.5) * env_tau;
  }
  return EXCENV_OK;
}

// The trajectory calls of the PMSM take one step per action row
template <class M> static int pmsm_one_substep(int32_t substeps) {
  if (M::IS_PMSM && substeps != 1) {
    set_error("PMSM: obs_stepsize must equal action_stepsize (reference pmsm_env.py:787)");
    return EXCENV_EUNSUPPORTED;
  }
  return EXCENV_OK;
}

// What the reverse launchers start from: broadcast properties (anything else is refused under the entry point's name `fn`), the
// dead-time coefficient and the step sizes in the element type. Args: VjpParamArgs, StepVjpArgs or StepJacArgs.
template <typename T, class M, template <typename, class> class Args>
static int reverse_preamble(const char* fn, Args<T, M>& ka, const excenv_props_t* props, double dt, double env_tau, bool ahead) {
  if (fill_props<T, M>(ka.kp, props)) {
    set_error("%s: per-environment property arrays are not supported", fn);
    return EXCENV_EUNSUPPORTED;
  }
  double coef;
  if (int rc = pmsm_coef<M>(props, env_tau, &coef, ahead)) return rc;
  ka.dt = (T)dt;
  ka.env_tau = (T)env_tau;
  ka.adv_coef = (T)coef;
  return EXCENV_OK;
}

template <class M, typename T> static int launch_step(const StepCall& sc) {
  StepArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  const bool batched = fill_props<T, M>(ka.kp, sc.props);
  double coef;
  if (int rc = pmsm_coef<M>(sc.props, sc.tau, &coef)) return rc;
  ka.B = sc.B;
  for (int j = 0; j < M::S; ++j) {
    if (!sc.state_in[j] || !sc.state_out[j]) { set_error("excenv_step: state pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.state_in[j] = (const T*)sc.state_in[j];
    ka.state_out[j] = (T*)sc.state_out[j];
  }
  ka.action = (const T*)sc.action;
  ka.obs = (T*)sc.obs;
  ka.n_control = sc.control ? sc.control->n_control : 0;
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = sc.control->control_idx[j];
    ka.reference[j] = (const T*)sc.control->reference[j];
    ka.obs_reference[j] = sc.control->obs_reference[j] ? (const T*)sc.control->obs_reference[j] : ka.reference[j];
  }
  ka.dt = (T)sc.tau;
  ka.env_tau = (T)sc.tau;
  ka.adv_coef = (T)coef;
  ka.reward = (T*)sc.reward;
  ka.terminated = (uint8_t*)sc.terminated;
  ka.truncated = (uint8_t*)sc.truncated;
  if (!aligned16(ka.action) || !aligned16(ka.obs)) {
    set_error("excenv_step: action and obs must be 16-byte aligned");
    return EXCENV_EINVAL;
  }
  if (sc.B == 0) return EXCENV_OK;
  constexpr int VMAX = 16 / (int)sizeof(T);
  const bool general = batched || ka.n_control > 0 || ka.reward != nullptr;
  int V = 1;
  if (!general) {
    bool ok = true;
    for (int j = 0; j < M::S; ++j) ok &= aligned16(ka.state_in[j]) && aligned16(ka.state_out[j]);
    int want = sc.vec_pref > 0 ? sc.vec_pref : 1;  // measured: one env per lane is fastest on this path
    if (want > VMAX) want = VMAX;
    while (want > 1 && (sc.B % want) != 0) want >>= 1;
    if (ok) V = want;
  }
  const int64_t lanes = sc.B / V;
  const dim3 grid((unsigned)((lanes + BLOCK - 1) / BLOCK)), block(BLOCK);
  // the DENSE observation path of step_kernel (kernels.hpp) stages BLOCK rows in static LDS: tables that would not fit next to
  // it stay in global memory (L2) instead of failing the launch
  constexpr int VWs = 16 / (int)sizeof(T);
  const bool dense = !general && V == 1 && (M::O % VWs) == 0 && (M::O / VWs) > 1;
  const size_t step_lds = lut_lds_bytes<T, M>(ka.kp, 0, dense ? sizeof(T) * BLOCK * M::O : 0);
  with_solver(sc.solver, [&](auto solver) {
    constexpr int SOLVER = decltype(solver)::value;
    if (general) launch_dyn(&step_kernel<M, T, SOLVER, true, 1>, grid, block, step_lds, sc.stream, ka);
    else with_const<1, 2, 4>(V, [&](auto v) {
      constexpr int VV = decltype(v)::value;
      if constexpr (VV <= VMAX) launch_dyn(&step_kernel<M, T, SOLVER, false, VV>, grid, block, step_lds, sc.stream, ka);
      return true;
    });
    return true;
  });
  g_last_launch = general ? "step_kernel (general)" : V == 1 ? "step_kernel (V=1)" : V == 2 ? "step_kernel (V=2)" : "step_kernel (V=4)";
  return check_launch("excenv_step");
}

// The trajectory kernels, one launcher per family. Each emits the instantiations sim_instantiated() (sim_plan.hpp) admits and no
// other, and returns whether the plan named one of them. SEM: the semantics (the clock of the lane-major kernels).
//
// The lane-major kernel (kernels.hpp): sim_ahead_kernel, or sim_ahead_acc_t_kernel on the accumulated-time clock. The plan gives
// the key (form, V, threads); STATES and LUT_LDS are the launch's own: general without / with the gym outputs' code (-2 / -1), lean
// without / with state trajectories (0 / 1); look-up models one instantiation per place the tables live in (LDS when they fit,
// lut_lds_bytes above).
template <class M, typename T, int SOLVER, int SEM>
static bool launch_lane_major(const SimPlan& p, SimArgs<T, M> ka, size_t lds_pad, T acc_step, T acc_end, hipStream_t stream) {
  constexpr bool ACC_T = SEM == EXCENV_SEM_AHEAD_ACCUMULATED_T;
  const size_t lds = lut_lds_bytes<T, M>(ka.kp, lds_pad);
  return with_const<SIM_GENERAL, SIM_LEAN, SIM_LEAN_GYM, SIM_AEM>(p.form, [&](auto form) {
    return with_const<1, 2, 4>(p.V, [&](auto v) {
      return with_const<BLOCK, WIDE_THREADS>(p.threads, [&](auto nt) {
        constexpr SimForm F = (SimForm)decltype(form)::value;
        constexpr int V = decltype(v)::value, NT = decltype(nt)::value;
        constexpr bool GEN = F == SIM_GENERAL;
        if constexpr (!sim_instantiated(SimPlan{F, false, V, NT, 0, 0, false, 0, ACC_T}, SEM, M::ID, M::A, (int)sizeof(T), SOLVER,
                                        M::HAS_LUT)) {
          return false;
        } else {
          const dim3 grid((unsigned)((ka.B / V + NT - 1) / NT)), block(NT);
          const size_t l = F == SIM_AEM ? aem_lds_bytes<M, T, V>() + lds : lds;  // AEM: the per-wave LDS piece ring of the actions
          with_flag(GEN ? ka.truncated != nullptr : ka.straj[0] != nullptr, [&](auto st) {
            return with_flag(ka.kp.lut_lds != 0, [&](auto lut_lds) {
              constexpr int STATES = (GEN ? -2 : 0) + decltype(st)::value;
              constexpr bool LUT_LDS = M::HAS_LUT && decltype(lut_lds)::value;
              if constexpr (ACC_T)
                launch_dyn(&sim_ahead_acc_t_kernel<M, T, SOLVER, GEN, V, STATES, LUT_LDS, NT>, grid, block, l, stream, ka, acc_step, acc_end);
              else
                launch_dyn(&sim_ahead_kernel<M, T, SOLVER, SEM == EXCENV_SEM_AHEAD, GEN, V, STATES, LUT_LDS, F == SIM_AEM, F == SIM_LEAN_GYM, NT>,
                           grid, block, l, stream, ka);
              return true;
            });
          });
          return true;
        }
      });
    });
  });
}

// The LDS-ring env-major kernel (kernels_em.hpp): one wave per 64 environments, TK steps staged in LDS, per-env contiguous runs
template <class M, typename T, int SOLVER, int SEM>
static bool launch_em(const SimPlan& p, const SimArgs<T, M>& ka, hipStream_t stream) {
  if constexpr (!sim_instantiated(SimPlan{SIM_EM, false, 1, EM_LANES, 0, 0, false, 0}, SEM, M::ID, M::A, (int)sizeof(T), SOLVER, M::HAS_LUT)) {
    return false;
  } else {
    const size_t lds = em_lds_elems((int)sizeof(T), M::S, M::O) * sizeof(T);
    const dim3 grid((unsigned)((ka.B + EM_LANES - 1) / EM_LANES)), block(EM_LANES);
    return with_flag(p.form == SIM_EM_GENERAL, [&](auto general) {
      launch_dyn(&sim_ahead_em_kernel<M, T, SOLVER, SEM == EXCENV_SEM_AHEAD, decltype(general)::value>, grid, block, lds, stream, ka);
      return true;
    });
  }
}

// The register-ring env-major kernel (kernels_emr.hpp): whole-line stores, lanes p.period environments apart (ka.a_wg)
template <class M, typename T, int SOLVER, int SEM>
static bool launch_emr(const SimPlan& p, const SimArgs<T, M>& ka, hipStream_t stream) {
  if constexpr (!sim_instantiated(SimPlan{SIM_EMR, false, 1, EM_LANES, 0, 0, false, 0}, SEM, M::ID, M::A, (int)sizeof(T), SOLVER, M::HAS_LUT)) {
    return false;
  } else {
    constexpr bool AHEAD = SEM == EXCENV_SEM_AHEAD;
    const int64_t per = EM_LANES * p.period;
    const dim3 grid((unsigned)(((ka.B + per - 1) / per) * p.period)), block(EM_LANES);
    launch_dyn(&sim_ahead_emr_kernel<M, T, SOLVER, AHEAD>, grid, block, emr_lds_bytes<M, T, AHEAD>(), stream, ka);
    return true;
  }
}

// Validates the call, packs SimArgs and launches the form sc.plan names
template <class M, typename T> static int launch_sim(const SimCall& sc) {
  SimArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, sc.props);
  double coef;
  if (int rc = pmsm_coef<M>(sc.props, sc.env_tau, &coef, sc.semantics != EXCENV_SEM_STEP)) return rc;
  if (int rc = pmsm_one_substep<M>(sc.substeps)) return rc;
  ka.B = sc.B;
  ka.K = sc.K;
  ka.substeps = sc.substeps;
  ka.n_control = sc.control ? sc.control->n_control : 0;
  const int64_t N = sc.K * sc.substeps;
  const int64_t OW = M::O + ka.n_control;
  const bool with_gym = sc.gym != nullptr;
  for (int j = 0; j < M::S; ++j) {
    if (!sc.state_in[j] || !sc.last_state[j]) { set_error("excenv_sim_ahead: state pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.state_in[j] = (const T*)sc.state_in[j];
    ka.last_state[j] = (T*)sc.last_state[j];
    ka.straj[j] = sc.state_traj ? (T*)sc.state_traj[j] : nullptr;
    if (sc.state_traj && !sc.state_traj[j]) { set_error("excenv_sim_ahead: state_traj pointer %d is NULL", j); return EXCENV_ENULL; }
  }
  ka.actions = (const T*)sc.actions;
  ka.obs = (T*)sc.obs_traj;
  constexpr int64_t TILE = EXCENV_TILE;  // envs per tile of the tiled layout (== one workgroup at V = TILE/BLOCK)
  if (sc.action_layout == EXCENV_LAYOUT_ENV_MAJOR) { ka.a_sb = sc.K * M::A; ka.a_sk = M::A; ka.a_sc = 1; }
  else if (sc.action_layout == EXCENV_LAYOUT_TILED) { ka.a_sb = 1; ka.a_sk = (int64_t)M::A * TILE; ka.a_sc = TILE; }
  else { ka.a_sb = 1; ka.a_sk = (int64_t)M::A * sc.B; ka.a_sc = sc.B; }
  if (sc.traj_layout == EXCENV_LAYOUT_ENV_MAJOR) {
    ka.o_sb = (N + 1) * OW; ka.o_sk = OW; ka.o_sc = 1;
    ka.s_sb = N + 1; ka.s_sk = 1;
  } else if (sc.traj_layout == EXCENV_LAYOUT_TILED) {
    ka.o_sb = 1; ka.o_sk = OW * TILE; ka.o_sc = TILE;
    ka.s_sb = 1; ka.s_sk = TILE;
  } else {
    ka.o_sb = 1; ka.o_sk = OW * sc.B; ka.o_sc = sc.B;
    ka.s_sb = 1; ka.s_sk = sc.B;
  }
  const bool tiled_a = sc.action_layout == EXCENV_LAYOUT_TILED, tiled_t = sc.traj_layout == EXCENV_LAYOUT_TILED;
  if ((tiled_a || tiled_t) && (sc.B % TILE) != 0) {
    set_error("excenv_sim_ahead: the tiled layout needs batch_size %% %lld == 0", (long long)TILE);
    return EXCENV_EINVAL;
  }
  if (with_gym) {
    if (!sc.gym->reward || !sc.gym->terminated || !sc.gym->truncated) {
      set_error("excenv_sim_ahead: gym trajectories need all of reward, terminated and truncated");
      return EXCENV_ENULL;
    }
    if (tiled_t) { set_error("excenv_sim_ahead: gym trajectories are not available in the tiled layout"); return EXCENV_EUNSUPPORTED; }
    const int64_t TW = (M::IS_PMSM || M::ID == EXCENV_FLUID_TANK) ? 1 : OW;
    ka.reward = (T*)sc.gym->reward;
    ka.terminated = sc.gym->terminated;
    ka.truncated = sc.gym->truncated;
    if (sc.traj_layout == EXCENV_LAYOUT_ENV_MAJOR) {
      ka.g_sb = N; ka.g_sk = 1;
      ka.t_sb = (N + 1) * TW; ka.t_sk = TW; ka.t_sc = 1;
    } else {
      ka.g_sb = 1; ka.g_sk = sc.B;
      ka.t_sb = TW; ka.t_sk = TW * sc.B; ka.t_sc = 1;  // lane-major flags: [row][B][TW], an environment's flags adjacent (ABI 7)
    }
  }
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = sc.control->control_idx[j];
    ka.reference[j] = (const T*)sc.control->reference[j];
  }
  ka.dt = (T)sc.obs_stepsize;
  ka.env_tau = (T)sc.env_tau;
  ka.adv_coef = (T)coef;
  ka.lin_stop = (T)(sc.env_tau * (double)(sc.K > 0 ? sc.K - 1 : 0));
  if (sc.B == 0) return EXCENV_OK;
  {  // per-lane offsets are 32-bit: 256 lanes * env stride * element size must stay below 2^31
    const int64_t lim = ((int64_t)1 << 31) / (BLOCK * (int64_t)sizeof(T));
    if (ka.a_sb >= lim || ka.o_sb >= lim || ka.s_sb >= lim) {
      set_error("excenv_sim_ahead: env-major trajectory too long for one call ((N+1)*O must be < %lld); chunk K",
                (long long)lim);
      return EXCENV_EUNSUPPORTED;
    }
  }

  const SimPlan& p = sc.plan;
  const bool emr = p.form == SIM_EMR, env_major = emr || p.form == SIM_EM || p.form == SIM_EM_GENERAL;
  if (emr) ka.a_wg = p.period;
  if (!env_major) {
    ka.row_sync = p.row_sync;
    // time-constant columns may stay as an earlier launch left them (sim_ahead_body.inc): lane-major rows, adjacent environments
    ka.keep_const = (sc.keep_const && sc.traj_layout == EXCENV_LAYOUT_LANE_MAJOR && ka.o_sb == 1 && ka.s_sb == 1) ? 1 : 0;
    // element offset of workgroup w's first env in each stream
    const int64_t wg_envs = (int64_t)p.threads * p.V;
    auto wg_off = [&](int layout, int64_t sb, int64_t per_tile) -> int64_t {
      if (layout == EXCENV_LAYOUT_TILED) return (wg_envs == TILE) ? per_tile : -1;
      return wg_envs * sb;
    };
    ka.a_wg = wg_off(sc.action_layout, ka.a_sb, sc.K * M::A * TILE);
    ka.o_wg = wg_off(sc.traj_layout, ka.o_sb, (N + 1) * OW * TILE);
    ka.s_wg = wg_off(sc.traj_layout, ka.s_sb, (N + 1) * TILE);
    if (ka.a_wg < 0 || ka.o_wg < 0 || ka.s_wg < 0) {
      set_error("excenv_sim_ahead: tiled layout needs unbatched properties, no gym trajectories, 16-byte aligned buffers and the %d-byte dtype (control columns are filled by a second launch)", 4);
      return EXCENV_EUNSUPPORTED;
    }
  }
  const size_t lds_pad = (size_t)sc.lds_pad + p.row_lds;
  // the accumulated-time clock's action step and end time, folded in double as oracle_body.inc does
  const T acc_step = (T)(sc.obs_stepsize * (double)sc.substeps), acc_end = (T)((sc.obs_stepsize * (double)sc.substeps) * (double)sc.K);
  auto launch = [&](auto solver, auto sem) {
    constexpr int SOLVER = decltype(solver)::value, SEM = decltype(sem)::value;
    if (emr) return launch_emr<M, T, SOLVER, SEM>(p, ka, sc.stream);
    if (env_major) return launch_em<M, T, SOLVER, SEM>(p, ka, sc.stream);
    return launch_lane_major<M, T, SOLVER, SEM>(p, ka, lds_pad, acc_step, acc_end, sc.stream);
  };
  if (!sim_instantiated(p, sc.semantics, M::ID, M::A, (int)sizeof(T), sc.solver, M::HAS_LUT) || !with_solver(sc.solver, [&](auto solver) {
        return with_const<EXCENV_SEM_STEP, EXCENV_SEM_AHEAD, EXCENV_SEM_AHEAD_ACCUMULATED_T>(sc.semantics, [&](auto sem) { return launch(solver, sem); });
      })) {
    set_error("excenv_sim_ahead: no kernel instantiation for plan '%s' (semantics %d, %d-byte elements)", plan_name(p), sc.semantics,
              (int)sizeof(T));
    return EXCENV_EINVAL;
  }
  g_last_launch = plan_name(p);
  if (int rc = check_launch(emr ? "excenv_sim_ahead (env-major fused, register ring)" : env_major ? "excenv_sim_ahead (env-major fused)" : "excenv_sim_ahead"))
    return rc;
  if (p.split_control) {
    ControlFillArgs<T, M> fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.kp = ka.kp;
    fa.B = sc.B;
    fa.rows = N + 1;
    fa.n_control = ka.n_control;
    fa.tiled = tiled_t ? 1 : 0;
    for (int j = 0; j < ka.n_control; ++j) {
      fa.control_idx[j] = ka.control_idx[j];
      fa.reference[j] = ka.reference[j];
    }
    fa.obs = ka.obs;
    fa.o_sk = ka.o_sk;
    fa.o_sc = ka.o_sc;
    fa.tile_pitch = (N + 1) * OW * TILE;
    bool v4 = (sizeof(T) == 4) && (sc.B % 4 == 0) && aligned16(ka.obs);
    for (int j = 0; j < ka.n_control; ++j) v4 &= aligned16(fa.reference[j]);
    const int64_t lanes = v4 ? sc.B / 4 : sc.B;
    const dim3 fgrid((unsigned)((lanes + BLOCK - 1) / BLOCK), (unsigned)((N + 1 < 64) ? N + 1 : 64)), fblock(BLOCK);
    if (v4) {
      if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((control_fill_kernel<M, T, 4>), fgrid, fblock, 0, sc.stream, fa);
    } else {
      hipLaunchKernelGGL((control_fill_kernel<M, T, 1>), fgrid, fblock, 0, sc.stream, fa);
    }
    return check_launch("excenv_sim_ahead (control columns)");
  }
  return EXCENV_OK;
}

template <class M, typename T> static int launch_traj_gym(const TrajGymCall& gc) {
  TrajGymArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, gc.props);
  ka.B = gc.B;
  ka.rows = gc.rows;
  ka.n_control = gc.control ? gc.control->n_control : 0;
  for (int j = 0; j < ka.n_control; ++j) {
    ka.control_idx[j] = gc.control->control_idx[j];
    ka.reference[j] = (const T*)gc.control->reference[j];
    ka.r_sb[j] = gc.ref_strides ? gc.ref_strides[2 * j] : 1;
    ka.r_sk[j] = gc.ref_strides ? gc.ref_strides[2 * j + 1] : 0;
  }
  for (int j = 0; j < M::S; ++j) {
    if (!gc.state_traj[j]) { set_error("excenv_rew_trunc_term: state_traj pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.straj[j] = (const T*)gc.state_traj[j];
  }
  ka.s_sb = gc.s_sb;
  ka.s_sk = gc.s_sk;
  ka.reward = (T*)gc.reward;
  ka.terminated = gc.terminated;
  ka.truncated = gc.truncated;
  const int64_t N = gc.rows - 1;
  const int64_t TW = (M::IS_PMSM || M::ID == EXCENV_FLUID_TANK) ? 1 : M::O + ka.n_control;
  if (gc.out_layout == EXCENV_LAYOUT_ENV_MAJOR) {
    ka.g_sb = N; ka.g_sk = 1;
    ka.t_sb = gc.rows * TW; ka.t_sk = TW; ka.t_sc = 1;
  } else {
    ka.g_sb = 1; ka.g_sk = gc.B;
    ka.t_sb = TW; ka.t_sk = TW * gc.B; ka.t_sc = 1;  // [row][B][TW]
  }
  if (gc.B == 0 || gc.rows == 0) return EXCENV_OK;
  ka.fast_is_env = (gc.s_sb == 1 || gc.rows == 1) ? 1 : 0;  // lanes run along the contiguous index of the state arrays
  const int64_t nfast = ka.fast_is_env ? gc.B : gc.rows, nslow = ka.fast_is_env ? gc.rows : gc.B;
  const int64_t blocks = ((nfast + BLOCK - 1) / BLOCK) * nslow;
  if (blocks >= ((int64_t)1 << 31)) { set_error("excenv_rew_trunc_term: trajectory too large for one launch"); return EXCENV_EUNSUPPORTED; }
  hipLaunchKernelGGL((traj_gym_kernel<M, T>), dim3((unsigned)blocks), dim3(BLOCK), 0, gc.stream, ka);
  return check_launch("excenv_rew_trunc_term");
}

template <class M, typename T> static int launch_from_obs(const FromObsCall& fc) {
  FromObsArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, fc.props);
  ka.B = fc.B;
  ka.n_control = fc.n_control;
  ka.obs = (const T*)fc.obs;
  for (int j = 0; j < M::S; ++j) {
    if (!fc.state_out[j]) { set_error("excenv_state_from_observation: state_out pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.state_out[j] = (T*)fc.state_out[j];
  }
  for (int j = 0; j < fc.n_control; ++j) {
    if (!fc.reference_out || !fc.reference_out[j]) { set_error("excenv_state_from_observation: reference_out pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.control_idx[j] = fc.control_idx[j];
    ka.reference_out[j] = (T*)fc.reference_out[j];
  }
  if (fc.B == 0) return EXCENV_OK;
  hipLaunchKernelGGL((from_obs_kernel<M, T>), dim3((unsigned)((fc.B + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, fc.stream, ka);
  return check_launch("excenv_state_from_observation");
}

template <class M, typename T> static int launch_observe(const ObserveCall& oc) {
  ObserveArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, oc.props);
  ka.B = oc.B;
  ka.n_control = oc.control ? oc.control->n_control : 0;
  ka.obs = (T*)oc.obs;
  for (int j = 0; j < M::S; ++j) {
    if (!oc.state[j]) { set_error("excenv_observe: state pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.state[j] = (const T*)oc.state[j];
  }
  for (int j = 0; j < ka.n_control; ++j) {
    if (!oc.control->reference[j]) { set_error("excenv_observe: reference pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.control_idx[j] = oc.control->control_idx[j];
    ka.reference[j] = (const T*)oc.control->reference[j];
  }
  if (oc.B == 0) return EXCENV_OK;
  hipLaunchKernelGGL((observe_kernel<M, T>), dim3((unsigned)((oc.B + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, oc.stream, ka);
  return check_launch("excenv_observe");
}

template <class M, typename T> static int launch_update_ref(const RefGenCall& rc) {
  RefGenArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, rc.props);
  ka.B = rc.B;
  ka.n_control = rc.n_control;
  for (int j = 0; j < rc.n_control; ++j) {
    if (!rc.reference[j]) { set_error("excenv_update_ref: reference pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.control_idx[j] = rc.control_idx[j];
    ka.reference[j] = (T*)rc.reference[j];
    ka.reference_in[j] = rc.reference_in ? (const T*)rc.reference_in[j] : (const T*)rc.reference[j];
    if (!ka.reference_in[j]) { set_error("excenv_update_ref: reference_in pointer %d is NULL", j); return EXCENV_ENULL; }
  }
  ka.keys = rc.keys;
  ka.hold = rc.hold;
  ka.keys_in = rc.keys_in ? rc.keys_in : rc.keys;
  ka.hold_in = rc.hold_in ? rc.hold_in : rc.hold;
  ka.hold_min = rc.hold_min;
  ka.hold_max = rc.hold_max;
  if (rc.B == 0) return EXCENV_OK;
  hipLaunchKernelGGL((update_ref_kernel<M, T>), dim3((unsigned)((rc.B + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, rc.stream, ka);
  return check_launch("excenv_update_ref");
}

template <class M, typename T> static int launch_random_state(const RandomStateCall& rc) {
  RandomStateArgs<T, M> ka;
  std::memset(&ka, 0, sizeof(ka));
  fill_props<T, M>(ka.kp, rc.props);
  ka.B = rc.B;
  ka.keys = rc.keys;
  ka.key_leaf = rc.key_leaf;
  for (int j = 0; j < M::S; ++j) {
    if (!rc.state_out[j]) { set_error("excenv_random_state: state_out pointer %d is NULL", j); return EXCENV_ENULL; }
    ka.state_out[j] = (T*)rc.state_out[j];
  }
  if (rc.B == 0) return EXCENV_OK;
  hipLaunchKernelGGL((random_state_kernel<M, T>), dim3((unsigned)((rc.B + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, rc.stream, ka);
  return check_launch("excenv_random_state");
}

template <template <typename> class MT> struct EnvEntry {
  static int step(const StepCall& sc) { return EXCENV_BY_DTYPE(launch_step, MT, sc); }
  static int sim(const SimCall& sc) { return EXCENV_BY_DTYPE(launch_sim, MT, sc); }
  static int traj_gym(const TrajGymCall& gc) { return EXCENV_BY_DTYPE(launch_traj_gym, MT, gc); }
  static int from_obs(const FromObsCall& fc) { return EXCENV_BY_DTYPE(launch_from_obs, MT, fc); }
  static int update_ref(const RefGenCall& rc) { return EXCENV_BY_DTYPE(launch_update_ref, MT, rc); }
  static int random_state(const RandomStateCall& rc) { return EXCENV_BY_DTYPE(launch_random_state, MT, rc); }
  static int observe(const ObserveCall& oc) { return EXCENV_BY_DTYPE(launch_observe, MT, oc); }
  static EnvVTable vtable() {
    return EnvVTable{MT<float>::S, MT<float>::A, MT<float>::O, MT<float>::P, &step, &sim, &traj_gym, &from_obs, &update_ref,
                     &random_state, &observe, &vjp_entry<MT>, &rew_vjp_entry<MT>, &step_vjp_entry<MT>, &step_jac_entry<MT>,
                     &feedback_entry<MT>, &feedback_vjp_entry<MT>, &policy_entry<MT>, &policy_episodes_entry<MT>, &policy_vjp_entry<MT>};
  }
};

// ---- rollout statistics on lane-major rows: excenv_row_moments, excenv_episode_stats --------------------------------
// row_moments_kernel<T>, episode_stats_kernel<T> and rollout_stats_reduce_kernel (rollout_stats.hip): no model, one instantiation per type
constexpr const char* row_moments_name() { return "row_moments_kernel"; }
constexpr const char* episode_stats_name() { return "episode_stats_kernel"; }
constexpr int STATS_BLOCK = 256;  // four waves: the moments' tiles are the PPO kernels' (PPO_LANE samples a lane), the scan has one environment per lane
static_assert(STATS_BLOCK == PPO_BLOCK, "a tile of the moments is a PPO tile");
// Rows of loads a lane of episode_stats_kernel keeps in flight ahead of the scan
constexpr int EPISODE_DEPTH = 8;

int launch_row_moments(int dtype, int64_t B, int64_t N, const excenv_row_moments_t& call, hipStream_t stream);
int launch_episode_stats(int dtype, int64_t B, int64_t K, const excenv_episode_stats_t& call, hipStream_t stream);

// One partial set per workgroup: functions of (B, N, C, max_groups) and of B only
inline int64_t row_moments_workspace(int64_t B, int64_t N, int C, int32_t max_groups) { return ppo_groups(B, N, max_groups) * (1 + 2 * C) * 8; }
inline int64_t episode_stats_groups(int64_t B) { return (B + STATS_BLOCK - 1) / STATS_BLOCK; }
inline int64_t episode_stats_workspace(int64_t B) { return episode_stats_groups(B) * EXCENV_EPISODE_STATS * 8; }

// What the two entries refuse: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values.
inline int stats_common_refusal(const char* fn, int dtype, int64_t B, int64_t K, const char* rows, char* msg, size_t n) {
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) {
    std::snprintf(msg, n, "%s: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got %d)", fn, dtype);
    return EXCENV_EINVAL;
  }
  if (B < 0 || K < 0) {
    std::snprintf(msg, n, "%s: bad B=%lld or %s=%lld", fn, (long long)B, rows, (long long)K);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}
inline int stats_workspace_refusal(const char* fn, const void* workspace, int64_t have, int64_t need, char* msg, size_t n) {
  if (have < need || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) {
    std::snprintf(msg, n, "%s: needs an 8-byte aligned workspace of %lld bytes (%s_workspace_bytes)", fn, (long long)need, fn);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}
inline int row_moments_refusal(int dtype, int64_t B, int64_t N, const excenv_row_moments_t* c, char* msg, size_t n) {
  const char* fn = "excenv_row_moments";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  if (!c->x) return null("call->x");
  if (!c->stats) return null("call->stats");
  if (!c->workspace) return null("call->workspace");
  if (int rc = stats_common_refusal(fn, dtype, B, N, "N", msg, n)) return rc;
  if (c->n_columns < 1 || c->n_columns > EXCENV_MOMENTS_MAX_COLUMNS) {
    std::snprintf(msg, n, "%s: call->n_columns must be 1 .. %d (got %d)", fn, EXCENV_MOMENTS_MAX_COLUMNS, c->n_columns);
    return EXCENV_EINVAL;
  }
  if (c->max_groups < 0) {
    std::snprintf(msg, n, "%s: call->max_groups must not be negative (got %d; 0: auto)", fn, c->max_groups);
    return EXCENV_EINVAL;
  }
  if (N > (int64_t)0x7fffffff / c->n_columns) {
    std::snprintf(msg, n, "%s: N * n_columns = %lld * %d rows exceed one launch", fn, (long long)N, c->n_columns);
    return EXCENV_EINVAL;
  }
  return stats_workspace_refusal(fn, c->workspace, c->workspace_bytes, row_moments_workspace(B, N, c->n_columns, c->max_groups), msg, n);
}
inline int episode_stats_refusal(int dtype, int64_t B, int64_t K, const excenv_episode_stats_t* c, char* msg, size_t n) {
  const char* fn = "excenv_episode_stats";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  if (!c->reward) return null("call->reward");
  if (!c->reset) return null("call->reset");
  if (!c->stats) return null("call->stats");
  if (!c->workspace) return null("call->workspace");
  if (int rc = stats_common_refusal(fn, dtype, B, K, "K", msg, n)) return rc;
  if (episode_stats_groups(B) >= ((int64_t)1 << 31)) {
    std::snprintf(msg, n, "%s: batch too large for one launch", fn);
    return EXCENV_EUNSUPPORTED;
  }
  return stats_workspace_refusal(fn, c->workspace, c->workspace_bytes, episode_stats_workspace(B), msg, n);
}

}  // namespace excenv
