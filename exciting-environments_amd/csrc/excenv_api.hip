// extern "C" entry points of libexcenv_hip.so (declared in include/excenv.h): argument validation,
// per-thread error string, dispatch into the per-environment launch tables. No device allocation,
// no synchronisation — only kernel enqueues on the caller's stream.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <dlfcn.h>
#include "launch.hpp"
#include "riccati.hpp"

static_assert(EXCENV_FAULT == 0, "EXCENV_FAULT builds exist for tools/isa_guards_selftest.sh only (single objects, never linked into the library)");

namespace excenv {

static thread_local char g_err[512] = "";
thread_local const char* g_last_launch = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int launch_transpose(int dtype, int64_t M, int64_t N, const void* in, void* out, hipStream_t stream);
int launch_param_sum(int dtype, int64_t B, int n, const void* const* per_env, void* out, void* workspace, hipStream_t stream);
int launch_policy_param_grad(int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_policy_param_grad_t& call, hipStream_t stream);
int launch_policy_eval(int dtype, int64_t B, int64_t R, int64_t row_stride, const excenv_policy_eval_t& call, hipStream_t stream);
int launch_gae(int dtype, int64_t B, int64_t K, const excenv_gae_t& call, hipStream_t stream);
int launch_gaussian_logp(int dtype, int64_t B, int64_t K, const excenv_gaussian_logp_t& call, hipStream_t stream);
int launch_ppo_loss(bool grad, int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t& call, hipStream_t stream);

EnvVTable vtable_pendulum();
EnvVTable vtable_msd();
EnvVTable vtable_cartpole();
EnvVTable vtable_acrobot();
EnvVTable vtable_tank();
EnvVTable vtable_pmsm();
EnvVTable vtable_pmsm_sat();

static const EnvVTable* table(int env) {
  static const EnvVTable T[EXCENV_NUM_ENVS + 1] = {vtable_pendulum(), vtable_msd(),  vtable_cartpole(), vtable_acrobot(),
                                                   vtable_tank(),     vtable_pmsm(), vtable_pmsm_sat()};
  if (env < 0 || env > EXCENV_NUM_ENVS) return nullptr;
  return &T[env];
}

static const EnvVTable* table_public(int env) { return (env >= 0 && env < EXCENV_NUM_ENVS) ? table(env) : nullptr; }

// Launch table for a call: PMSM with LUTs attached runs the saturated model's instantiations.
static const EnvVTable* table_for(int env, const excenv_props_t* props, int* rc) {
  *rc = EXCENV_OK;
  if (env < 0 || env >= EXCENV_NUM_ENVS) return nullptr;
  if (props && props->pmsm_lut) {
    const excenv_pmsm_lut_t* l = props->pmsm_lut;
    if (env != EXCENV_PMSM) { set_error("pmsm_lut is only valid for EXCENV_PMSM"); *rc = EXCENV_EINVAL; return nullptr; }
    if (l->n_d < 2 || l->n_q < 2 || !l->grid_d || !l->grid_q || !l->tables) {
      set_error("pmsm_lut: need n_d, n_q >= 2 and non-NULL grid / table pointers");
      *rc = EXCENV_EINVAL;
      return nullptr;
    }
    return table(EXCENV_NUM_ENVS);
  }
  return table(env);
}

static const excenv_launch_opts_t kDefaultOpts = {0, 0, 0, 0};  // envs_per_lane, env_major_mode, lds_pad_bytes, flags

static int check_opts(const char* fn, const excenv_launch_opts_t*& o) {
  if (!o) o = &kDefaultOpts;
  const int v = o->envs_per_lane;
  if (!(v == 0 || v == 1 || v == 2 || v == 4)) { set_error("%s: opts.envs_per_lane must be 0, 1, 2 or 4 (got %d)", fn, v); return EXCENV_EINVAL; }
  if (o->env_major_mode < 0 || o->env_major_mode > 3) { set_error("%s: opts.env_major_mode must be 0, 1, 2 or 3", fn); return EXCENV_EINVAL; }
  if (o->lds_pad_bytes < 0 || o->lds_pad_bytes > 150 * 1024) { set_error("%s: opts.lds_pad_bytes out of range", fn); return EXCENV_EINVAL; }
  if ((o->flags & ~(EXCENV_OPT_NO_FUSED_ACTIONS | EXCENV_OPT_KEEP_CONSTANT_COLUMNS)) != 0) { set_error("%s: opts.flags has unknown bits set (0x%x)", fn, (unsigned)o->flags); return EXCENV_EINVAL; }
  return EXCENV_OK;
}

static int check_common(const char* fn, int env, int solver, int dtype, int64_t B) {
  if (env < 0 || env >= EXCENV_NUM_ENVS) { set_error("%s: bad env id %d", fn, env); return EXCENV_EINVAL; }
  if (solver < 0 || solver >= EXCENV_NUM_SOLVERS) { set_error("%s: bad solver id %d", fn, solver); return EXCENV_EINVAL; }
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) { set_error("%s: bad dtype id %d", fn, dtype); return EXCENV_EINVAL; }
  if (B < 0 || B > ((int64_t)1 << 31) * BLOCK) { set_error("%s: bad batch size %lld", fn, (long long)B); return EXCENV_EINVAL; }
  return EXCENV_OK;
}

static int check_n_control(const char* fn, int n_control) {
  if (n_control < 0 || n_control > EXCENV_MAX_CONTROL) { set_error("%s: bad n_control %d", fn, n_control); return EXCENV_EINVAL; }
  return EXCENV_OK;
}
// The controlled fields are state leaves of the model: field j alone (for callers that check more of field j before field j + 1), or all
static int check_control_idx_at(const char* fn, int env, int j, int32_t idx) {
  if (idx < 0 || idx >= table_public(env)->S) { set_error("%s: control_idx[%d] out of range", fn, j); return EXCENV_EINVAL; }
  return EXCENV_OK;
}
static int check_control_idx(const char* fn, int env, int n_control, const int32_t* control_idx) {
  for (int j = 0; j < n_control; ++j)
    if (int rc = check_control_idx_at(fn, env, j, control_idx[j])) return rc;
  return EXCENV_OK;
}

static int check_control(const char* fn, int env, const excenv_control_t*& c) {
  if (c && c->n_control == 0) c = nullptr;
  if (!c) return EXCENV_OK;
  if (int rc = check_n_control(fn, c->n_control)) return rc;
  for (int j = 0; j < c->n_control; ++j) {
    if (int rc = check_control_idx_at(fn, env, j, c->control_idx[j])) return rc;
    if (!c->reference[j]) { set_error("%s: reference[%d] is NULL", fn, j); return EXCENV_ENULL; }
  }
  return EXCENV_OK;
}

// Is any property of the model a per-environment array?
static bool props_per_env(const EnvVTable* t, const excenv_props_t* props) {
  bool per_env = false;
  for (int j = 0; j < t->P; ++j) per_env |= props->static_params[j].per_env != nullptr;
  for (int j = 0; j < t->S; ++j) per_env |= props->state_min[j].per_env != nullptr || props->state_max[j].per_env != nullptr;
  for (int j = 0; j < t->A; ++j) per_env |= props->action_min[j].per_env != nullptr || props->action_max[j].per_env != nullptr;
  return per_env;
}

// What every reverse-mode call asks of its properties, in two parts because the calls check other arguments in between
static int check_reverse_props(const char* fn, const excenv_props_t* props) {
  if (!props) { set_error("%s: props is NULL", fn); return EXCENV_ENULL; }
  if (props->pmsm_lut) { set_error("%s: the saturated PMSM (pmsm_lut) has no reverse mode", fn); return EXCENV_EUNSUPPORTED; }
  return EXCENV_OK;
}
static int check_broadcast_props(const char* fn, int env, const excenv_props_t* props) {
  if (props_per_env(table_public(env), props)) { set_error("%s: per-environment property arrays are not supported (broadcast properties only)", fn); return EXCENV_EUNSUPPORTED; }
  return EXCENV_OK;
}

// What the closed-loop calls (excenv_sim_feedback, excenv_sim_policy, excenv_sim_feedback_vjp) check alike, in parts because each
// checks its policy or call record and the control block in between, in its own order. The head:
static int check_closed_loop_head(const char* fn, int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps) {
  if (int rc = check_common(fn, env, solver, dtype, B)) return rc;
  if (K < 0 || substeps < 1) { set_error("%s: bad K=%lld or substeps=%d", fn, (long long)K, substeps); return EXCENV_EINVAL; }
  return EXCENV_OK;
}
// The arguments a forward rollout cannot do without
static int check_rollout_pointers(const char* fn, const excenv_props_t* props, const void* state_in, const void* obs_traj, const void* last_state) {
  if (!props) { set_error("%s: props is NULL", fn); return EXCENV_ENULL; }
  if (!state_in) { set_error("%s: state_in is NULL", fn); return EXCENV_ENULL; }
  if (!obs_traj) { set_error("%s: obs_traj is NULL", fn); return EXCENV_ENULL; }
  if (!last_state) { set_error("%s: last_state is NULL", fn); return EXCENV_ENULL; }
  return EXCENV_OK;
}
// The tail: the launch options, the one form these kernels have, one step per action row for the PMSM
static int check_closed_loop_tail(const char* fn, int env, int32_t substeps, const excenv_launch_opts_t*& opts) {
  if (int rc = check_opts(fn, opts)) return rc;
  if (opts->envs_per_lane > 1) {
    set_error("%s: opts.envs_per_lane = %d is not available (this kernel has the one-environment-per-lane form only)", fn, opts->envs_per_lane);
    return EXCENV_EINVAL;
  }
  if (env == EXCENV_PMSM && substeps != 1) {
    set_error("%s: PMSM: obs_stepsize must equal action_stepsize (substeps = %d; reference pmsm_env.py:787)", fn, substeps);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

}  // namespace excenv

using namespace excenv;

extern "C" {

int excenv_abi_version(void) { return EXCENV_ABI_VERSION; }

const char* excenv_last_error(void) { return g_err; }

const char* excenv_last_launch(void) { return g_last_launch; }

int excenv_env_dims(int env, int32_t* S, int32_t* A, int32_t* O, int32_t* P) {
  const EnvVTable* t = table_public(env);
  if (!t) { set_error("excenv_env_dims: bad env id %d", env); return EXCENV_EINVAL; }
  if (S) *S = t->S;
  if (A) *A = t->A;
  if (O) *O = t->O;
  if (P) *P = t->P;
  return EXCENV_OK;
}

int64_t excenv_step_bytes(int env, int dtype) {
  const EnvVTable* t = table_public(env);
  if (!t) return -1;
  const int64_t w = dtype == EXCENV_F64 ? 8 : 4;
  return w * (t->S + t->A + t->S + t->O);
}

int64_t excenv_sim_ahead_bytes(int env, int dtype, int with_state_traj) {
  const EnvVTable* t = table_public(env);
  if (!t) return -1;
  const int64_t w = dtype == EXCENV_F64 ? 8 : 4;
  return w * (t->A + t->O + (with_state_traj ? t->S : 0));
}

int excenv_step(int env, int solver, int dtype, int64_t B, const excenv_props_t* props,
                const excenv_control_t* control, double tau, const void* const* state_in, const void* action,
                void* const* state_out, void* obs, const excenv_launch_opts_t* opts, void* stream) {
  if (int rc = check_common("excenv_step", env, solver, dtype, B)) return rc;
  if (!props || !state_in || !action || !state_out || !obs) { set_error("excenv_step: NULL argument"); return EXCENV_ENULL; }
  if (int rc = check_control("excenv_step", env, control)) return rc;
  if (int rc = check_opts("excenv_step", opts)) return rc;
  StepCall sc{opts->envs_per_lane, solver, dtype, B, props, control, tau, state_in, action, state_out, obs, nullptr, nullptr, nullptr,
              (hipStream_t)stream};
  int rc;
  const EnvVTable* vt = table_for(env, props, &rc);
  return vt ? vt->step(sc) : rc;
}

int32_t excenv_truncated_width(int env, int32_t n_control) {
  const EnvVTable* t = table_public(env);
  if (!t || n_control < 0) return -1;
  return (env == EXCENV_FLUID_TANK || env == EXCENV_PMSM) ? 1 : t->O + n_control;
}

int excenv_gym_step(int env, int solver, int dtype, int64_t B, const excenv_props_t* props,
                    const excenv_control_t* control, double tau, const void* const* state_in, const void* action,
                    void* const* state_out, void* obs, void* reward, uint8_t* terminated, uint8_t* truncated,
                    const excenv_launch_opts_t* opts, void* stream) {
  if (int rc = check_common("excenv_gym_step", env, solver, dtype, B)) return rc;
  if (!props || !state_in || !action || !state_out || !obs || !reward || !terminated || !truncated) {
    set_error("excenv_gym_step: NULL argument");
    return EXCENV_ENULL;
  }
  if (int rc = check_control("excenv_gym_step", env, control)) return rc;
  if (int rc = check_opts("excenv_gym_step", opts)) return rc;
  StepCall sc{1, solver, dtype, B, props, control, tau, state_in, action, state_out, obs, reward, terminated, truncated,
              (hipStream_t)stream};
  int rc;
  const EnvVTable* vt = table_for(env, props, &rc);
  return vt ? vt->step(sc) : rc;
}

int64_t excenv_sim_ahead_workspace_bytes(int env, int dtype, int64_t B, int64_t K, int32_t substeps, int32_t n_control,
                                         int action_layout, int traj_layout, int with_state_traj) {
  const EnvVTable* t = table_public(env);
  if (!t || B < 0 || K < 0 || substeps < 1 || n_control < 0) return -1;
  return sim_workspace_bytes(t->S, t->A, t->O, dtype == EXCENV_F64 ? 8 : 4, B, K, substeps, n_control, action_layout, traj_layout,
                             with_state_traj != 0);
}

// The facts sim_plan() decides a call's form from
static SimFacts sim_facts(int env, const EnvVTable* t, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                          const excenv_props_t* props, int n_control, int semantics, int action_layout, int traj_layout,
                          const excenv_launch_opts_t* opts) {
  SimFacts f{};
  f.env = env; f.S = t->S; f.A = t->A; f.O = t->O; f.elem = dtype == EXCENV_F64 ? 8 : 4; f.solver = solver; f.semantics = semantics;
  f.B = B; f.K = K; f.substeps = substeps; f.action_layout = action_layout; f.traj_layout = traj_layout;
  f.per_env_props = props_per_env(t, props);
  f.lut = props->pmsm_lut != nullptr; f.n_control = n_control; f.refs_given = true;
  f.al_actions = f.al_obs = f.al_state_io = f.al_straj = f.al_reward = f.al_terminated = f.al_truncated = f.al_refs = 128;
  f.envs_per_lane = opts->envs_per_lane; f.env_major_mode = opts->env_major_mode; f.flags = opts->flags;
  return f;
}

int excenv_sim_ahead_fuses_actions(int env, int solver, int dtype, int64_t B, int64_t K, const excenv_props_t* props,
                                   int32_t n_control, int with_gym, int action_layout, int traj_layout, const void* actions,
                                   const excenv_launch_opts_t* opts) {
  if (check_common("excenv_sim_ahead_fuses_actions", env, solver, dtype, B) || !props) return 0;
  if (check_opts("excenv_sim_ahead_fuses_actions", opts)) return 0;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return 0;
  // what the query cannot see is assumed (include/excenv.h): references given, state and trajectory arrays 16-byte aligned
  SimFacts f = sim_facts(env, t, solver, dtype, B, K, 1, props, n_control, EXCENV_SEM_STEP, action_layout, traj_layout, opts);
  f.gym = with_gym != 0;
  f.al_actions = align_of(actions);
  f.al_obs = f.al_state_io = f.al_straj = 16;
  return sim_plan(f).form == SIM_AEM ? 1 : 0;
}

int excenv_transpose(int dtype, int64_t M, int64_t N, const void* in, void* out, void* stream) {
  if ((dtype != EXCENV_F32 && dtype != EXCENV_F64) || M < 0 || N < 0) { set_error("excenv_transpose: bad argument"); return EXCENV_EINVAL; }
  if ((!in || !out) && M * N > 0) { set_error("excenv_transpose: NULL argument"); return EXCENV_ENULL; }
  int rc = launch_transpose(dtype, M, N, in, out, (hipStream_t)stream);
  if (rc) set_error("excenv_transpose: launch failed");
  return rc;
}

int excenv_sim_ahead_ws(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                        const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                        double env_tau, const void* const* state_in, const void* actions, int action_layout,
                        void* obs_traj, void* const* state_traj, int traj_layout, void* const* last_state,
                        int semantics, const excenv_traj_gym_t* gym, void* workspace, int64_t workspace_bytes,
                        const excenv_launch_opts_t* opts, void* stream) {
  if (int rc = check_common("excenv_sim_ahead", env, solver, dtype, B)) return rc;
  if (K < 0 || substeps < 1) { set_error("excenv_sim_ahead: bad K=%lld or substeps=%d", (long long)K, substeps); return EXCENV_EINVAL; }
  if (semantics != EXCENV_SEM_STEP && semantics != EXCENV_SEM_AHEAD && semantics != EXCENV_SEM_AHEAD_ACCUMULATED_T) {
    set_error("excenv_sim_ahead: bad semantics %d", semantics);
    return EXCENV_EINVAL;
  }
  if (semantics == EXCENV_SEM_AHEAD_ACCUMULATED_T && K >= ((int64_t)1 << 30)) {  // the clock's action rows are 32-bit (sim_clock.hpp)
    set_error("excenv_sim_ahead: EXCENV_SEM_AHEAD_ACCUMULATED_T needs K < 2^30 (got %lld)", (long long)K);
    return EXCENV_EUNSUPPORTED;
  }
  if (action_layout < EXCENV_LAYOUT_ENV_MAJOR || action_layout > EXCENV_LAYOUT_TILED ||
      traj_layout < EXCENV_LAYOUT_ENV_MAJOR || traj_layout > EXCENV_LAYOUT_TILED) {
    set_error("excenv_sim_ahead: bad layout id");
    return EXCENV_EINVAL;
  }
  if (!props || !state_in || (!actions && K > 0) || !obs_traj || !last_state) { set_error("excenv_sim_ahead: NULL argument"); return EXCENV_ENULL; }
  if (int rc = check_control("excenv_sim_ahead", env, control)) return rc;
  if (int rc = check_opts("excenv_sim_ahead", opts)) return rc;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  const int nc = control ? control->n_control : 0;
  SimFacts f = sim_facts(env, t, solver, dtype, B, K, substeps, props, nc, semantics, action_layout, traj_layout, opts);
  f.gym = gym != nullptr; f.state_traj = state_traj != nullptr; f.al_actions = align_of(actions); f.al_obs = align_of(obs_traj);
  for (int j = 0; j < t->S; ++j) {
    f.al_state_io = std::min(f.al_state_io, std::min(align_of(state_in[j]), align_of(last_state[j])));
    if (state_traj) f.al_straj = std::min(f.al_straj, align_of(state_traj[j]));
  }
  if (gym) { f.al_reward = align_of(gym->reward); f.al_terminated = align_of(gym->terminated); f.al_truncated = align_of(gym->truncated); }
  for (int j = 0; j < nc; ++j) f.al_refs = std::min(f.al_refs, align_of(control->reference[j]));  // non-NULL (check_control)
  f.workspace = workspace != nullptr; f.al_workspace = align_of(workspace); f.workspace_bytes = workspace_bytes;
  const SimPlan plan = sim_plan(f);
  SimCall sc{solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, state_in, actions, action_layout,
             obs_traj, state_traj, traj_layout, last_state, semantics, opts->lds_pad_bytes, gym, (hipStream_t)stream, plan};
  // the caller's promise about its own lane-major output buffers (a trajectory workspace holds no earlier launch's rows)
  sc.keep_const = (opts->flags & EXCENV_OPT_KEEP_CONSTANT_COLUMNS) != 0 && traj_layout == EXCENV_LAYOUT_LANE_MAJOR;
  if (!plan.via_workspace) return t->sim(sc);
  // env-major buffers + workspace: transpose in, run the coalesced lane-major kernel, transpose out
  const int64_t w = f.elem, N = K * substeps, OW = t->O + nc;
  char* ws = (char*)workspace;
  void* k_straj[EXCENV_MAX_STATE] = {nullptr};
  sc.plan.via_workspace = false;  // what runs on the workspace
  if (action_layout == EXCENV_LAYOUT_ENV_MAJOR) {
    if (int rc = launch_transpose(dtype, B, K * t->A, actions, ws, sc.stream)) { set_error("excenv_sim_ahead: action transpose failed"); return rc; }
    sc.actions = ws;
    sc.action_layout = EXCENV_LAYOUT_LANE_MAJOR;
    ws += align_up(w * K * t->A * B);
  }
  if (traj_layout == EXCENV_LAYOUT_ENV_MAJOR) {
    sc.obs_traj = ws;
    ws += align_up(w * (N + 1) * OW * B);
    if (state_traj) {
      for (int j = 0; j < t->S; ++j) { k_straj[j] = ws; ws += align_up(w * (N + 1) * B); }
      sc.state_traj = k_straj;
    }
    sc.traj_layout = EXCENV_LAYOUT_LANE_MAJOR;
  }
  if (int rc = t->sim(sc)) return rc;
  g_last_launch = plan_name(plan);
  if (traj_layout == EXCENV_LAYOUT_ENV_MAJOR) {
    if (int rc = launch_transpose(dtype, (N + 1) * OW, B, sc.obs_traj, obs_traj, sc.stream)) { set_error("excenv_sim_ahead: obs transpose failed"); return rc; }
    if (state_traj)
      for (int j = 0; j < t->S; ++j)
        if (int rc = launch_transpose(dtype, N + 1, B, k_straj[j], state_traj[j], sc.stream)) { set_error("excenv_sim_ahead: state transpose failed"); return rc; }
  }
  return EXCENV_OK;
}

int excenv_sim_ahead(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                     const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                     double env_tau, const void* const* state_in, const void* actions, int action_layout,
                     void* obs_traj, void* const* state_traj, int traj_layout, void* const* last_state,
                     int semantics, const excenv_traj_gym_t* gym, const excenv_launch_opts_t* opts, void* stream) {
  return excenv_sim_ahead_ws(env, solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, state_in, actions,
                             action_layout, obs_traj, state_traj, traj_layout, last_state, semantics, gym, nullptr, 0, opts,
                             stream);
}

int64_t excenv_sim_ahead_vjp_workspace_bytes(int env, int dtype, int64_t B, int64_t K, int action_layout) {
  const EnvVTable* t = table_public(env);
  if (!t || B < 0 || K < 0) return -1;
  return vjp_workspace_bytes(t->A, dtype == EXCENV_F64 ? 8 : 4, B, K, action_layout);
}

int64_t excenv_sim_ahead_vjp_workspace_bytes_for(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                                                 int semantics, int action_layout) {
  const EnvVTable* t = table_public(env);
  if (!t || B < 0 || K < 0 || substeps < 1) return -1;
  const int elem = dtype == EXCENV_F64 ? 8 : 4;
  return vjp_workspace_bytes(t->A, elem, B, K, action_layout) + vjp_raw_rows_bytes(env, solver, semantics, elem, B, K, substeps);
}

}  // extern "C"

// excenv_sim_ahead_vjp (grad_params == nullptr, pgrad false) and excenv_sim_ahead_vjp_params: one validation, one launch
static int sim_ahead_vjp_call(const char* fn, bool pgrad, int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                              const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                              double env_tau, const void* actions, int action_layout, const void* const* state_traj,
                              const void* grad_obs_traj, const void* const* grad_state_traj,
                              const void* const* grad_last_state, void* grad_actions, void* const* grad_state_in,
                              int semantics, void* workspace, int64_t workspace_bytes, const excenv_launch_opts_t* opts,
                              void* stream, void* const* grad_params) {
  if (int rc = check_common(fn, env, solver, dtype, B)) return rc;
  if (K < 0 || substeps < 1) { set_error("%s: bad K=%lld or substeps=%d", fn, (long long)K, substeps); return EXCENV_EINVAL; }
  if (semantics == EXCENV_SEM_AHEAD_ACCUMULATED_T) {
    set_error("%s: EXCENV_SEM_AHEAD_ACCUMULATED_T has no reverse mode (use EXCENV_SEM_AHEAD or EXCENV_SEM_STEP)", fn);
    return EXCENV_EUNSUPPORTED;
  }
  if (semantics != EXCENV_SEM_STEP && semantics != EXCENV_SEM_AHEAD) { set_error("%s: bad semantics %d", fn, semantics); return EXCENV_EINVAL; }
  if (action_layout == EXCENV_LAYOUT_TILED) { set_error("%s: the tiled layout has no reverse mode (lane-major or env-major actions)", fn); return EXCENV_EUNSUPPORTED; }
  if (action_layout != EXCENV_LAYOUT_ENV_MAJOR && action_layout != EXCENV_LAYOUT_LANE_MAJOR) { set_error("%s: bad layout id", fn); return EXCENV_EINVAL; }
  if (!props || !state_traj || !grad_state_in || ((!actions || !grad_actions) && K > 0)) { set_error("%s: NULL argument", fn); return EXCENV_ENULL; }
  if (int rc = check_reverse_props(fn, props)) return rc;
  const EnvVTable* t = table_public(env);
  bool params_aligned = true;
  if (pgrad) {
    if (!grad_params) { set_error("%s: NULL argument", fn); return EXCENV_ENULL; }
    bool any = false;
    for (int j = 0; j < EXCENV_MAX_STATIC; ++j) {
      if (!grad_params[j]) continue;
      if (j >= t->P) { set_error("%s: grad_params[%d]: this model has %d static parameters", fn, j, t->P); return EXCENV_EINVAL; }
      if (!vjp_param_differentiable(env, j)) { set_error("%s: grad_params[%d]: static parameter %d is an integer leaf and has no gradient", fn, j, j); return EXCENV_EINVAL; }
      any = true;
      params_aligned = params_aligned && align_of(grad_params[j]) >= 16;
    }
    if (!any) { set_error("%s: every entry of grad_params is NULL (excenv_sim_ahead_vjp is the call without parameter gradients)", fn); return EXCENV_EINVAL; }
  }
  const int nc = control ? control->n_control : 0;
  if (int rc = check_n_control(fn, nc)) return rc;
  if (int rc = check_opts(fn, opts)) return rc;
  if (int rc = check_broadcast_props(fn, env, props)) return rc;
  const int elem = dtype == EXCENV_F64 ? 8 : 4;
  const void* k_actions = actions;
  const bool transposed = action_layout == EXCENV_LAYOUT_ENV_MAJOR && B > 0 && K > 0;
  if (transposed) {
    const int64_t need = vjp_workspace_bytes(t->A, elem, B, K, action_layout);
    if (!workspace || workspace_bytes < need) {
      set_error("%s: env-major actions need a workspace of %lld bytes (excenv_sim_ahead_vjp_workspace_bytes)", fn, (long long)need);
      return EXCENV_EINVAL;
    }
    k_actions = workspace;
  }
  void* raw_rows = nullptr;
  if (B > 0 && K > 0 && vjp_needs_raw_rows(env, solver, semantics)) {
    const int64_t head = transposed ? vjp_workspace_bytes(t->A, elem, B, K, action_layout) : 0;
    const int64_t need = head + vjp_raw_rows_bytes(env, solver, semantics, elem, B, K, substeps);
    if (!workspace || workspace_bytes < need) {
      set_error("%s: this model, solver and semantics need a workspace of %lld bytes (excenv_sim_ahead_vjp_workspace_bytes_for)", fn, (long long)need);
      return EXCENV_EINVAL;
    }
    raw_rows = (char*)workspace + head;
  }
  // the wide form: whole lanes and 16-byte accesses everywhere
  bool wide_ok = params_aligned && (B % (16 / elem)) == 0 && align_of(k_actions) >= 16 && align_of(grad_actions) >= 16 && align_of(grad_obs_traj) >= 16;
  for (int j = 0; j < t->S; ++j) {
    if (!state_traj[j] || !grad_state_in[j]) { set_error("%s: state pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    wide_ok = wide_ok && align_of(state_traj[j]) >= 16 && align_of(grad_state_in[j]) >= 16 &&
              (!grad_state_traj || align_of(grad_state_traj[j]) >= 16) && (!grad_last_state || align_of(grad_last_state[j]) >= 16);
  }
  const int V = vjp_envs_per_lane(env, solver, B, elem, opts->envs_per_lane, wide_ok, pgrad);
  if (V == 0 || !vjp_instantiated(semantics, env, elem, solver, false, V, pgrad)) {
    set_error("%s: opts.envs_per_lane = %d is not available (1, or %d where the model and solver have that form, with batch_size %% %d == 0 and 16-byte aligned arrays)", fn,
              opts->envs_per_lane, 16 / elem, 16 / elem);
    return EXCENV_EINVAL;
  }
  if (transposed) {
    if (int rc = launch_transpose(dtype, B, K * t->A, actions, workspace, (hipStream_t)stream)) { set_error("%s: action transpose failed", fn); return rc; }
  }
  const VjpCall vc{solver, dtype, B, K, substeps, nc, props, obs_stepsize, env_tau, semantics, k_actions, state_traj, grad_obs_traj,
                   grad_state_traj, grad_last_state, grad_actions, grad_state_in, V, raw_rows, stream, pgrad ? grad_params : nullptr};
  return t->sim_vjp(vc);
}

extern "C" {

int excenv_sim_ahead_vjp(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                         const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                         double env_tau, const void* actions, int action_layout, const void* const* state_traj,
                         const void* grad_obs_traj, const void* const* grad_state_traj,
                         const void* const* grad_last_state, void* grad_actions, void* const* grad_state_in,
                         int semantics, void* workspace, int64_t workspace_bytes, const excenv_launch_opts_t* opts,
                         void* stream) {
  return sim_ahead_vjp_call("excenv_sim_ahead_vjp", false, env, solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau,
                            actions, action_layout, state_traj, grad_obs_traj, grad_state_traj, grad_last_state, grad_actions,
                            grad_state_in, semantics, workspace, workspace_bytes, opts, stream, nullptr);
}

int excenv_sim_ahead_vjp_params(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                                const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                                double env_tau, const void* actions, int action_layout, const void* const* state_traj,
                                const void* grad_obs_traj, const void* const* grad_state_traj,
                                const void* const* grad_last_state, void* grad_actions, void* const* grad_state_in,
                                int semantics, void* workspace, int64_t workspace_bytes, const excenv_launch_opts_t* opts,
                                void* stream, void* const* grad_params) {
  return sim_ahead_vjp_call("excenv_sim_ahead_vjp_params", true, env, solver, dtype, B, K, substeps, props, control, obs_stepsize,
                            env_tau, actions, action_layout, state_traj, grad_obs_traj, grad_state_traj, grad_last_state,
                            grad_actions, grad_state_in, semantics, workspace, workspace_bytes, opts, stream, grad_params);
}

int excenv_param_differentiable(int env, int index) {
  const EnvVTable* t = table_public(env);
  if (!t || index < 0 || index >= t->P) return -1;
  return vjp_param_differentiable(env, index) ? 1 : 0;
}

int64_t excenv_param_grad_sum_workspace_bytes(int dtype, int64_t B, int32_t n) {
  if ((dtype != EXCENV_F32 && dtype != EXCENV_F64) || B < 0 || n < 0 || n > EXCENV_MAX_STATIC) return -1;
  return param_sum_workspace_bytes(B, n);
}

int excenv_param_grad_sum(int dtype, int64_t B, int32_t n, const void* const* per_env_ptrs, void* out, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  const char* fn = "excenv_param_grad_sum";
  if ((dtype != EXCENV_F32 && dtype != EXCENV_F64) || B < 0 || n < 0 || n > EXCENV_MAX_STATIC) { set_error("%s: bad argument", fn); return EXCENV_EINVAL; }
  if (n == 0) return EXCENV_OK;
  if (!per_env_ptrs || !out || !workspace) { set_error("%s: NULL argument", fn); return EXCENV_ENULL; }
  for (int j = 0; j < n; ++j)
    if (!per_env_ptrs[j] && B > 0) { set_error("%s: per_env_ptrs[%d] is NULL", fn, j); return EXCENV_ENULL; }
  const int64_t need = param_sum_workspace_bytes(B, n);
  if (workspace_bytes < need || align_of(workspace) < 8) {
    set_error("%s: needs an 8-byte aligned workspace of %lld bytes (excenv_param_grad_sum_workspace_bytes)", fn, (long long)need);
    return EXCENV_EINVAL;
  }
  int rc = launch_param_sum(dtype, B, n, per_env_ptrs, out, workspace, (hipStream_t)stream);
  if (rc) set_error("%s: launch failed", fn);
  return rc;
}

int excenv_rew_trunc_term(int env, int dtype, int64_t B, int64_t rows, const excenv_props_t* props,
                          const excenv_control_t* control, const int64_t* ref_strides, const void* const* state_traj,
                          int64_t state_env_stride, int64_t state_row_stride, void* reward, uint8_t* terminated,
                          uint8_t* truncated, int out_layout, void* stream) {
  if (int rc = check_common("excenv_rew_trunc_term", env, 0, dtype, B)) return rc;
  if (rows < 1) { set_error("excenv_rew_trunc_term: rows must be >= 1 (row 0 is the initial state)"); return EXCENV_EINVAL; }
  if (out_layout != EXCENV_LAYOUT_ENV_MAJOR && out_layout != EXCENV_LAYOUT_LANE_MAJOR) { set_error("excenv_rew_trunc_term: bad out_layout"); return EXCENV_EINVAL; }
  if (!props || !state_traj || !truncated || (rows > 1 && (!reward || !terminated))) { set_error("excenv_rew_trunc_term: NULL argument"); return EXCENV_ENULL; }
  if (int rc = check_control("excenv_rew_trunc_term", env, control)) return rc;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  TrajGymCall gc{dtype, B, rows, props, control, ref_strides, state_traj, state_env_stride, state_row_stride, reward,
                 terminated, truncated, out_layout, (hipStream_t)stream};
  return t->traj_gym(gc);
}

int excenv_rew_reads(int env, int32_t n_control, const int32_t* control_idx, uint8_t reads[EXCENV_MAX_STATE]) {
  const EnvVTable* t = table_public(env);
  if (!t) { set_error("excenv_rew_reads: bad env id %d", env); return EXCENV_EINVAL; }
  if (int rc = check_n_control("excenv_rew_reads", n_control)) return rc;
  if (!reads || (n_control > 0 && !control_idx)) { set_error("excenv_rew_reads: NULL argument"); return EXCENV_ENULL; }
  if (int rc = check_control_idx("excenv_rew_reads", env, n_control, control_idx)) return rc;
  uint8_t r[EXCENV_MAX_STATE];
  reward_reads(env, n_control, control_idx, r);
  std::copy(r, r + EXCENV_MAX_STATE, reads);
  return EXCENV_OK;
}

int excenv_rew_vjp(int env, int dtype, int64_t B, int64_t rows, const excenv_props_t* props,
                   const excenv_control_t* control, const int64_t* ref_strides, const void* const* state_traj,
                   int64_t state_env_stride, int64_t state_row_stride, const void* grad_reward, int64_t grad_env_stride,
                   int64_t grad_row_stride, void* const* grad_state_traj, const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_rew_vjp";
  if (int rc = check_common(fn, env, 0, dtype, B)) return rc;
  if (rows < 1) { set_error("%s: rows must be >= 1 (row 0 is the initial state)", fn); return EXCENV_EINVAL; }
  if (!props || !state_traj || !grad_state_traj || (rows > 1 && !grad_reward)) { set_error("%s: NULL argument", fn); return EXCENV_ENULL; }
  if (int rc = check_control(fn, env, control)) return rc;
  if (int rc = check_opts(fn, opts)) return rc;
  int trc;
  if (!table_for(env, props, &trc)) return trc;  // a malformed pmsm_lut is rejected as everywhere; a valid one is not read
  if (B == 0) return EXCENV_OK;  // nothing to write: no launch, whatever the (empty) arrays' addresses are
  const EnvVTable* t = table_public(env);
  const int nc = control ? control->n_control : 0;
  uint8_t reads[EXCENV_MAX_STATE];
  reward_reads(env, nc, control ? control->control_idx : nullptr, reads);
  const int elem = dtype == EXCENV_F64 ? 8 : 4;
  // the fast form: whole lanes, everything lane-major and 16-byte aligned, broadcast properties
  bool fast_ok = (B % (16 / elem)) == 0 && state_env_stride == 1 && state_row_stride == B &&
                 (rows == 1 || (grad_env_stride == 1 && grad_row_stride == B && align_of(grad_reward) >= 16));
  bool any = false;
  for (int j = 0; j < t->S; ++j) {
    if (!reads[j]) continue;
    any = true;
    if (!state_traj[j]) { set_error("%s: state_traj pointer %d is NULL (the reward reads this leaf)", fn, j); return EXCENV_ENULL; }
    if (!grad_state_traj[j]) { set_error("%s: grad_state_traj pointer %d is NULL (the reward reads this leaf)", fn, j); return EXCENV_ENULL; }
    fast_ok = fast_ok && align_of(state_traj[j]) >= 16 && align_of(grad_state_traj[j]) >= 16;
  }
  for (int j = 0; j < nc; ++j) {
    const int64_t sb = ref_strides ? ref_strides[2 * j] : 1, sk = ref_strides ? ref_strides[2 * j + 1] : 0;
    fast_ok = fast_ok && sb == 1 && (sk == 0 || sk == B) && align_of(control->reference[j]) >= 16;
  }
  fast_ok = fast_ok && !props_per_env(t, props);
  const int V = rew_vjp_envs_per_lane(elem, opts->envs_per_lane, fast_ok);
  if (V == 0) {
    set_error("%s: opts.envs_per_lane = %d is not available (1, or %d with lane-major 16-byte aligned arrays, batch_size %% %d == 0 and "
              "broadcast properties)", fn, opts->envs_per_lane, 16 / elem, 16 / elem);
    return EXCENV_EINVAL;
  }
  for (int j = 0; j < t->S; ++j)  // leaves the reward does not read have a zero cotangent
    if (!reads[j] && grad_state_traj[j]) {
      const hipError_t e = hipMemsetAsync(grad_state_traj[j], 0, (size_t)elem * (size_t)rows * (size_t)B, (hipStream_t)stream);
      if (e != hipSuccess) { set_error("%s: zero-fill of grad_state_traj[%d] failed: %s", fn, j, hipGetErrorString(e)); return EXCENV_EHIP; }
    }
  if (!any) {
    g_last_launch = "rew_vjp_kernel (nothing read: no launch)";
    return EXCENV_OK;
  }
  const RewVjpCall rc{dtype, B, rows, props, control, ref_strides, state_traj, state_env_stride, state_row_stride, grad_reward,
                      grad_env_stride, grad_row_stride, grad_state_traj, reads, V, stream};
  return t->rew_vjp(rc);
}

int64_t excenv_step_vjp_bytes(int env, int dtype, int32_t n_control, int has_grad_obs, int has_grad_state, int has_grad_reward) {
  const EnvVTable* t = table_public(env);
  if (!t || (dtype != EXCENV_F32 && dtype != EXCENV_F64) || n_control < 0 || n_control > EXCENV_MAX_CONTROL) return -1;
  return step_vjp_bytes(t->S, t->A, t->O, dtype == EXCENV_F64 ? 8 : 4, n_control, has_grad_obs != 0, has_grad_state != 0, has_grad_reward != 0);
}

int excenv_step_vjp(int env, int solver, int dtype, int64_t B, const excenv_props_t* props, const excenv_control_t* control,
                    double tau, const void* const* state_in, const void* action, const void* const* state_out,
                    const void* grad_obs, const void* const* grad_state_out, const void* grad_reward,
                    void* const* grad_state_in, void* grad_action, const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_step_vjp";
  if (int rc = check_common(fn, env, solver, dtype, B)) return rc;
  if (int rc = check_reverse_props(fn, props)) return rc;
  const EnvVTable* t = table_public(env);
  if (control && control->n_control == 0) control = nullptr;
  const int nc = control ? control->n_control : 0;
  if (int rc = check_n_control(fn, nc)) return rc;
  if (grad_reward) {  // the reward reads the controlled fields and their references; without any it is a constant
    if (!control) {
      set_error("%s: grad_reward without control references (the reward depends on the state through the controlled fields only)", fn);
      return EXCENV_EUNSUPPORTED;
    }
    for (int j = 0; j < nc; ++j) {
      if (int rc = check_control_idx_at(fn, env, j, control->control_idx[j])) return rc;
      if (!control->reference[j]) { set_error("%s: reference[%d] is NULL (grad_reward reads the references)", fn, j); return EXCENV_ENULL; }
    }
  }
  if (int rc = check_opts(fn, opts)) return rc;
  if (int rc = check_broadcast_props(fn, env, props)) return rc;
  if (B == 0) return EXCENV_OK;  // nothing to write: no launch, whatever the (empty) arrays' addresses are
  if (!state_in) { set_error("%s: state_in is NULL", fn); return EXCENV_ENULL; }
  if (!action) { set_error("%s: action is NULL", fn); return EXCENV_ENULL; }
  if (!state_out) { set_error("%s: state_out is NULL", fn); return EXCENV_ENULL; }
  if (!grad_state_in) { set_error("%s: grad_state_in is NULL", fn); return EXCENV_ENULL; }
  if (!grad_action) { set_error("%s: grad_action is NULL", fn); return EXCENV_ENULL; }
  for (int j = 0; j < t->S; ++j) {
    if (!state_in[j]) { set_error("%s: state_in pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    if (!state_out[j]) { set_error("%s: state_out pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    if (!grad_state_in[j]) { set_error("%s: grad_state_in pointer %d is NULL", fn, j); return EXCENV_ENULL; }
  }
  const int V = step_vjp_envs_per_lane(opts->envs_per_lane);
  if (V == 0) {
    set_error("%s: opts.envs_per_lane = %d is not available (this kernel has the one-environment-per-lane form only)", fn, opts->envs_per_lane);
    return EXCENV_EINVAL;
  }
  if (align_of(action) < 16 || align_of(grad_action) < 16 || align_of(grad_obs) < 16) {  // rows are read as 16-byte pieces
    set_error("%s: action, grad_action and grad_obs must be 16-byte aligned", fn);
    return EXCENV_EINVAL;
  }
  const StepVjpCall sc{solver, dtype, B, props, control, tau, state_in, action, state_out, grad_obs, grad_state_out, grad_reward,
                       grad_state_in, grad_action, V, stream};
  return t->step_vjp(sc);
}

int64_t excenv_step_jacobian_bytes(int env, int dtype, int row_kind) {
  const EnvVTable* t = table_public(env);
  if (!t || (dtype != EXCENV_F32 && dtype != EXCENV_F64) || (row_kind != EXCENV_JAC_STATE && row_kind != EXCENV_JAC_OBS)) return -1;
  return step_jac_bytes(t->S, t->A, t->O, dtype == EXCENV_F64 ? 8 : 4, row_kind);
}

int excenv_step_jacobian(int env, int solver, int dtype, int64_t B, int64_t rows, int32_t substeps, const excenv_props_t* props,
                         int32_t n_control, double dt, double env_tau, const void* const* state_in, const void* const* state_out,
                         int64_t state_row_stride, const void* action, int64_t action_row_stride, int64_t action_comp_stride,
                         int64_t action_env_stride, int row_kind, void* jacobian, const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_step_jacobian";
  if (int rc = check_common(fn, env, solver, dtype, B)) return rc;
  if (rows < 0) { set_error("%s: bad rows %lld", fn, (long long)rows); return EXCENV_EINVAL; }
  if (substeps < 1) { set_error("%s: bad substeps %d (at least 1)", fn, (int)substeps); return EXCENV_EINVAL; }
  if (int rc = check_n_control(fn, n_control)) return rc;
  if (row_kind != EXCENV_JAC_STATE && row_kind != EXCENV_JAC_OBS) { set_error("%s: bad row_kind %d", fn, row_kind); return EXCENV_EINVAL; }
  if (int rc = check_reverse_props(fn, props)) return rc;
  const EnvVTable* t = table_public(env);
  if (int rc = check_opts(fn, opts)) return rc;
  if (int rc = check_broadcast_props(fn, env, props)) return rc;
  const int V = step_jac_envs_per_lane(opts->envs_per_lane);
  if (V == 0) {
    set_error("%s: opts.envs_per_lane = %d is not available (this kernel has the one-instance-per-lane form only)", fn, opts->envs_per_lane);
    return EXCENV_EINVAL;
  }
  if (B == 0 || rows == 0) return EXCENV_OK;  // nothing to write: no launch, whatever the (empty) arrays' addresses are
  if (!state_in) { set_error("%s: state_in is NULL", fn); return EXCENV_ENULL; }
  if (!state_out) { set_error("%s: state_out is NULL", fn); return EXCENV_ENULL; }
  if (!action) { set_error("%s: action is NULL", fn); return EXCENV_ENULL; }
  if (!jacobian) { set_error("%s: jacobian is NULL", fn); return EXCENV_ENULL; }
  for (int j = 0; j < t->S; ++j) {
    if (!state_in[j]) { set_error("%s: state_in pointer %d is NULL", fn, j); return EXCENV_ENULL; }
    if (!state_out[j]) { set_error("%s: state_out pointer %d is NULL", fn, j); return EXCENV_ENULL; }
  }
  if (state_row_stride < 0 || action_row_stride < 0 || action_comp_stride < 0 || action_env_stride < 0) {
    set_error("%s: strides must not be negative", fn);
    return EXCENV_EINVAL;
  }
  const StepJacCall jc{solver, dtype, B, rows, substeps, props, dt, env_tau, state_in, state_out, state_row_stride, action,
                       action_row_stride, action_comp_stride, action_env_stride, row_kind, jacobian, V, stream};
  return t->step_jac(jc);
}

int excenv_sim_feedback(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                        const excenv_control_t* control, double obs_stepsize, double env_tau, const void* const* state_in,
                        const excenv_feedback_t* policy, void* obs_traj, void* const* state_traj, void* const* last_state,
                        void* actions_out, const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_sim_feedback";
  if (int rc = check_closed_loop_head(fn, env, solver, dtype, B, K, substeps)) return rc;
  if (int rc = check_rollout_pointers(fn, props, state_in, obs_traj, last_state)) return rc;
  {
    char why[256];
    if (int rc = feedback_policy_refusal(policy, B, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (int rc = check_control(fn, env, control)) return rc;
  if (int rc = check_closed_loop_tail(fn, env, substeps, opts)) return rc;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  const FeedbackCall fc{solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, state_in, policy, obs_traj, state_traj,
                        last_state, actions_out, stream};
  return t->sim_feedback(fc);
}

int64_t excenv_sim_feedback_vjp_workspace_bytes(int env, int dtype, int64_t B, int64_t K, int32_t n_control, int64_t gain_batch,
                                                int integral) {
  const EnvVTable* t = table_public(env);
  if (!t || (dtype != EXCENV_F32 && dtype != EXCENV_F64) || B < 0 || K < 0 || n_control < 0 || n_control > EXCENV_MAX_CONTROL) return -1;
  if (gain_batch != 1 && gain_batch != B) return -1;
  return feedback_vjp_workspace_bytes(t->A, t->O + n_control, dtype == EXCENV_F64 ? 8 : 4, B, K, gain_batch, integral != 0);
}

int64_t excenv_sim_feedback_vjp_bytes(int env, int dtype, int32_t n_control, int32_t substeps, int integral, int has_grad_obs,
                                      int has_grad_states, int has_grad_actions) {
  const EnvVTable* t = table_public(env);
  if (!t || (dtype != EXCENV_F32 && dtype != EXCENV_F64) || n_control < 0 || n_control > EXCENV_MAX_CONTROL || substeps < 1) return -1;
  return feedback_vjp_bytes(t->S, t->A, t->O, dtype == EXCENV_F64 ? 8 : 4, n_control, substeps, integral != 0, has_grad_obs != 0,
                            has_grad_states != 0, has_grad_actions != 0);
}

int excenv_sim_feedback_vjp(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                            const excenv_control_t* control, double obs_stepsize, double env_tau,
                            const excenv_feedback_vjp_t* call, void* workspace, int64_t workspace_bytes,
                            const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_sim_feedback_vjp";
  if (int rc = check_closed_loop_head(fn, env, solver, dtype, B, K, substeps)) return rc;
  if (int rc = check_reverse_props(fn, props)) return rc;
  {
    char why[256];
    if (int rc = feedback_vjp_refusal(call, B, K, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (int rc = check_control(fn, env, control)) return rc;
  if (int rc = check_closed_loop_tail(fn, env, substeps, opts)) return rc;
  if (int rc = check_broadcast_props(fn, env, props)) return rc;
  const EnvVTable* t = table_public(env);
  const int64_t need = feedback_vjp_workspace_bytes(t->A, t->O + (control ? control->n_control : 0), dtype == EXCENV_F64 ? 8 : 4, B, K,
                                                    call->gain_batch, call->integral_gain != nullptr);
  if (B > 0 && need > 0 && (!workspace || workspace_bytes < need)) {
    set_error("%s: workspace too small: %lld bytes needed (excenv_sim_feedback_vjp_workspace_bytes), %lld given", fn, (long long)need,
              (long long)(workspace ? workspace_bytes : 0));
    return EXCENV_EINVAL;
  }
  const FeedbackVjpCall fc{solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, call, workspace, stream};
  return t->sim_feedback_vjp(fc);
}

int excenv_sim_policy(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                      const excenv_control_t* control, double obs_stepsize, double env_tau, const void* const* state_in,
                      const excenv_policy_t* policy, void* obs_traj, void* const* state_traj, void* const* last_state,
                      void* actions_out, const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_sim_policy";
  if (int rc = check_closed_loop_head(fn, env, solver, dtype, B, K, substeps)) return rc;
  if (int rc = check_rollout_pointers(fn, props, state_in, obs_traj, last_state)) return rc;
  if (int rc = check_control(fn, env, control)) return rc;  // (before the policy: its first width is O + n_control)
  {
    char why[256];
    const EnvVTable* d = table_public(env);
    if (int rc = policy_refusal(policy, d->O + (control ? control->n_control : 0), d->A, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (int rc = check_closed_loop_tail(fn, env, substeps, opts)) return rc;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  const PolicyCall pc{solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, state_in, policy, obs_traj, state_traj,
                      last_state, actions_out, stream};
  return t->sim_policy(pc);
}

int excenv_sim_policy_episodes(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                               const excenv_control_t* control, double obs_stepsize, double env_tau, const void* const* state_in,
                               const excenv_policy_t* policy, void* obs_traj, void* const* state_traj, void* const* last_state,
                               void* actions_out, const excenv_episode_t* episode, const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_sim_policy_episodes";
  if (int rc = check_closed_loop_head(fn, env, solver, dtype, B, K, substeps)) return rc;
  if (int rc = check_rollout_pointers(fn, props, state_in, obs_traj, last_state)) return rc;
  if (int rc = check_control(fn, env, control)) return rc;  // (before the policy: its first width is O + n_control)
  const EnvVTable* d = table_public(env);
  {
    char why[256];
    if (int rc = policy_refusal(policy, d->O + (control ? control->n_control : 0), d->A, why, sizeof(why), fn)) { set_error("%s", why); return rc; }
  }
  if (int rc = check_closed_loop_tail(fn, env, substeps, opts)) return rc;
  {
    char why[256];
    if (int rc = episode_refusal(episode, d->S, substeps, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  const EpisodeCall ec{{solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, state_in, policy, obs_traj, state_traj,
                        last_state, actions_out, stream},
                       episode};
  return t->sim_policy_episodes(ec);
}

int64_t excenv_sim_policy_vjp_bytes(int env, int dtype, int32_t n_control, int32_t substeps, int has_grad_obs, int has_grad_states,
                                    int has_grad_actions, int has_reset) {
  const EnvVTable* t = table_public(env);
  if (!t || (dtype != EXCENV_F32 && dtype != EXCENV_F64) || n_control < 0 || n_control > EXCENV_MAX_CONTROL || substeps < 1) return -1;
  if (has_reset && substeps != 1) return -1;
  return policy_vjp_bytes(t->S, t->A, t->O, dtype == EXCENV_F64 ? 8 : 4, n_control, substeps, has_grad_obs != 0, has_grad_states != 0,
                          has_grad_actions != 0, has_reset != 0);
}

int excenv_sim_policy_vjp(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                          const excenv_control_t* control, double obs_stepsize, double env_tau, const excenv_policy_vjp_t* call,
                          const excenv_launch_opts_t* opts, void* stream) {
  const char* fn = "excenv_sim_policy_vjp";
  if (int rc = check_closed_loop_head(fn, env, solver, dtype, B, K, substeps)) return rc;
  if (int rc = check_reverse_props(fn, props)) return rc;
  if (!call) { set_error("%s: call is NULL", fn); return EXCENV_ENULL; }
  // (before the policy: its first width is O + n_control. Only the count is read — references get no gradient — so a control block
  // that carries nothing else is valid here, as for excenv_sim_ahead_vjp)
  if (control && control->n_control == 0) control = nullptr;
  if (control)
    if (int rc = check_n_control(fn, control->n_control)) return rc;
  const EnvVTable* t = table_public(env);
  {
    char why[256];
    if (int rc = policy_refusal(&call->policy, t->O + (control ? control->n_control : 0), t->A, why, sizeof(why), fn)) { set_error("%s", why); return rc; }
  }
  if (int rc = check_closed_loop_tail(fn, env, substeps, opts)) return rc;
  {
    char why[256];
    if (int rc = policy_vjp_refusal(call, K, substeps, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (int rc = check_broadcast_props(fn, env, props)) return rc;
  const PolicyVjpCall vc{solver, dtype, B, K, substeps, props, control, obs_stepsize, env_tau, call, stream};
  return t->sim_policy_vjp(vc);
}

int64_t excenv_policy_param_grad_workspace_bytes(int dtype, int64_t B, int64_t K, const excenv_policy_t* policy, int32_t max_groups) {
  if ((dtype != EXCENV_F32 && dtype != EXCENV_F64) || B < 0 || K < 0 || !policy || max_groups < 0) return -1;
  if (policy->n_layers < 1 || policy->n_layers > EXCENV_POLICY_MAX_LAYERS) return -1;
  for (int l = 0; l <= policy->n_layers; ++l)
    if (policy->widths[l] < 1 || policy->widths[l] > EXCENV_POLICY_MAX_WIDTH) return -1;
  return policy_param_grad_workspace(B, K, *policy, max_groups);
}

int excenv_policy_param_grad(int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_policy_param_grad_t* call, void* stream) {
  {
    char why[256];
    if (int rc = policy_param_grad_refusal(dtype, B, K, substeps, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0) return EXCENV_OK;
  return launch_policy_param_grad(dtype, B, K, substeps, *call, (hipStream_t)stream);
}

int excenv_policy_eval(int dtype, int64_t B, int64_t R, int64_t row_stride, const excenv_policy_eval_t* call, void* stream) {
  {
    char why[256];
    if (int rc = policy_eval_refusal(dtype, B, R, row_stride, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || R == 0) return EXCENV_OK;
  return launch_policy_eval(dtype, B, R, row_stride, *call, (hipStream_t)stream);
}

int excenv_gae(int dtype, int64_t B, int64_t K, const excenv_gae_t* call, void* stream) {
  {
    char why[256];
    if (int rc = gae_refusal(dtype, B, K, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || K == 0) return EXCENV_OK;
  return launch_gae(dtype, B, K, *call, (hipStream_t)stream);
}

int excenv_gaussian_logp(int dtype, int64_t B, int64_t K, const excenv_gaussian_logp_t* call, void* stream) {
  {
    char why[256];
    if (int rc = gaussian_logp_refusal(dtype, B, K, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || K == 0) return EXCENV_OK;
  return launch_gaussian_logp(dtype, B, K, *call, (hipStream_t)stream);
}

int64_t excenv_ppo_loss_workspace_bytes(int64_t B, int64_t K, int32_t max_groups) {
  if (B < 0 || K < 0 || max_groups < 0) return -1;
  return ppo_loss_workspace(B, K, max_groups);
}

int excenv_ppo_loss(int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t* call, void* stream) {
  {
    char why[256];
    if (int rc = ppo_loss_refusal(false, dtype, B, K, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || K == 0) return EXCENV_OK;
  return launch_ppo_loss(false, dtype, B, K, *call, (hipStream_t)stream);
}

int excenv_ppo_loss_grad(int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t* call, void* stream) {
  {
    char why[256];
    if (int rc = ppo_loss_refusal(true, dtype, B, K, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || K == 0) return EXCENV_OK;
  return launch_ppo_loss(true, dtype, B, K, *call, (hipStream_t)stream);
}

int64_t excenv_row_moments_workspace_bytes(int64_t B, int64_t N, int32_t n_columns, int32_t max_groups) {
  if (B < 0 || N < 0 || n_columns < 1 || n_columns > EXCENV_MOMENTS_MAX_COLUMNS || max_groups < 0) return -1;
  return row_moments_workspace(B, N, n_columns, max_groups);
}

int excenv_row_moments(int dtype, int64_t B, int64_t N, const excenv_row_moments_t* call, void* stream) {
  {
    char why[256];
    if (int rc = row_moments_refusal(dtype, B, N, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || N == 0) return EXCENV_OK;
  return launch_row_moments(dtype, B, N, *call, (hipStream_t)stream);
}

int64_t excenv_episode_stats_workspace_bytes(int64_t B) {
  if (B < 0 || episode_stats_groups(B) >= ((int64_t)1 << 31)) return -1;
  return episode_stats_workspace(B);
}

int excenv_episode_stats(int dtype, int64_t B, int64_t K, const excenv_episode_stats_t* call, void* stream) {
  {
    char why[256];
    if (int rc = episode_stats_refusal(dtype, B, K, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0 || K == 0) return EXCENV_OK;
  return launch_episode_stats(dtype, B, K, *call, (hipStream_t)stream);
}

int excenv_lqr_backward(int dtype, int64_t B, int64_t N, const excenv_lqr_t* call, void* stream) {
  {
    char why[256];
    if (int rc = riccati_refusal(dtype, B, N, call, why, sizeof(why))) { set_error("%s", why); return rc; }
  }
  if (B == 0) return EXCENV_OK;
  return launch_riccati(dtype, B, N, *call, (hipStream_t)stream);
}

int64_t excenv_lqr_backward_bytes(int dtype, int32_t n_state, int32_t n_action, int time_invariant, int has_q, int has_r, int store_all,
                                  int has_ff) {
  return riccati_bytes(dtype, n_state, n_action, time_invariant, has_q, has_r, store_all, has_ff);
}

int excenv_state_from_observation(int env, int dtype, int64_t B, const excenv_props_t* props, int32_t n_control,
                                  const int32_t* control_idx, const void* obs, void* const* state_out,
                                  void* const* reference_out, void* stream) {
  if (int rc = check_common("excenv_state_from_observation", env, 0, dtype, B)) return rc;
  if (int rc = check_n_control("excenv_state_from_observation", n_control)) return rc;
  if (!props || !obs || !state_out || (n_control > 0 && (!control_idx || !reference_out))) { set_error("excenv_state_from_observation: NULL argument"); return EXCENV_ENULL; }
  if (int rc = check_control_idx("excenv_state_from_observation", env, n_control, control_idx)) return rc;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  FromObsCall fc{dtype, B, props, n_control, control_idx, obs, state_out, reference_out, (hipStream_t)stream};
  return t->from_obs(fc);
}

int excenv_observe(int env, int dtype, int64_t B, const excenv_props_t* props, const excenv_control_t* control,
                   const void* const* state, void* obs, void* stream) {
  if (int rc = check_common("excenv_observe", env, 0, dtype, B)) return rc;
  if (!props || !state || !obs) { set_error("excenv_observe: NULL argument"); return EXCENV_ENULL; }
  if (control) {
    if (int rc = check_n_control("excenv_observe", control->n_control)) return rc;
    if (int rc = check_control_idx("excenv_observe", env, control->n_control, control->control_idx)) return rc;
  }
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  ObserveCall oc{dtype, B, props, control, state, obs, (hipStream_t)stream};
  return t->observe(oc);
}

int excenv_update_ref(int env, int dtype, int64_t B, const excenv_props_t* props, int32_t n_control,
                      const int32_t* control_idx, void* const* reference, int64_t* keys, int64_t* hold,
                      int32_t hold_steps_min, int32_t hold_steps_max, void* stream) {
  if (int rc = check_common("excenv_update_ref", env, 0, dtype, B)) return rc;
  if (int rc = check_n_control("excenv_update_ref", n_control)) return rc;
  if (!props || !keys || !hold || (n_control > 0 && (!control_idx || !reference))) { set_error("excenv_update_ref: NULL argument"); return EXCENV_ENULL; }
  if (int rc = check_control_idx("excenv_update_ref", env, n_control, control_idx)) return rc;
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  RefGenCall rc{dtype, B, props, n_control, control_idx, reference, keys, hold, hold_steps_min, hold_steps_max, (hipStream_t)stream};
  return t->update_ref(rc);
}

int excenv_update_ref_to(int env, int dtype, int64_t B, const excenv_props_t* props, int32_t n_control,
                         const int32_t* control_idx, const void* const* reference_in, const int64_t* keys_in,
                         const int64_t* hold_in, void* const* reference_out, int64_t* keys_out, int64_t* hold_out,
                         int32_t hold_steps_min, int32_t hold_steps_max, void* stream) {
  if (int rc = check_common("excenv_update_ref_to", env, 0, dtype, B)) return rc;
  if (int rc = check_n_control("excenv_update_ref_to", n_control)) return rc;
  if (!props || !keys_in || !hold_in || !keys_out || !hold_out || (n_control > 0 && (!control_idx || !reference_in || !reference_out))) {
    set_error("excenv_update_ref_to: NULL argument");
    return EXCENV_ENULL;
  }
  if (keys_in == keys_out || hold_in == hold_out) { set_error("excenv_update_ref_to: outputs must not alias the inputs (use excenv_update_ref)"); return EXCENV_EINVAL; }
  for (int j = 0; j < n_control; ++j) {
    if (int rc = check_control_idx_at("excenv_update_ref_to", env, j, control_idx[j])) return rc;
    if (reference_in[j] == reference_out[j]) { set_error("excenv_update_ref_to: outputs must not alias the inputs (use excenv_update_ref)"); return EXCENV_EINVAL; }
  }
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  RefGenCall rc{dtype, B, props, n_control, control_idx, reference_out, keys_out, hold_out, hold_steps_min, hold_steps_max,
                (hipStream_t)stream, reference_in, keys_in, hold_in};
  return t->update_ref(rc);
}

int excenv_random_state(int env, int dtype, int64_t B, const excenv_props_t* props, const int64_t* keys,
                        void* const* state_out, int64_t* key_leaf, void* stream) {
  if (int rc = check_common("excenv_random_state", env, 0, dtype, B)) return rc;
  if (!props || !keys || !state_out || !key_leaf) { set_error("excenv_random_state: NULL argument"); return EXCENV_ENULL; }
  int trc;
  const EnvVTable* t = table_for(env, props, &trc);
  if (!t) return trc;
  RandomStateCall rc{dtype, B, props, keys, state_out, key_leaf, (hipStream_t)stream};
  return t->random_state(rc);
}

// ---- the one collective of the path: reassemble observations on every rank -------------------------------
// RCCL is resolved at run time (dlopen: librccl.so, the library torch.distributed's "nccl" backend uses on ROCm) so that
// single-GPU users of libexcenv_hip.so do not need it; the communicator is the caller's.
namespace {
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
struct RcclEntry {
  nccl_allgather_fn fn = nullptr;
  const char* err = nullptr;
  RcclEntry() {
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* h = nullptr;
    for (const char* n : names) {
      h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (h) break;
    }
    if (!h) err = "librccl.so could not be loaded";
    else {
      fn = (nccl_allgather_fn)dlsym(h, "ncclAllGather");
      if (!fn) err = "librccl.so has no ncclAllGather";
    }
  }
};
nccl_allgather_fn resolve_allgather(const char** why) {
  static const RcclEntry entry;  // initialised once, thread-safely (C++11 function-local static); read-only afterwards
  if (why) *why = entry.err;
  return entry.fn;
}
}  // namespace

int excenv_allgather(void* nccl_comm, int dtype, const void* send, void* recv, int64_t count_per_rank, void* stream) {
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) { set_error("excenv_allgather: bad dtype id %d", dtype); return EXCENV_EINVAL; }
  if (count_per_rank < 0) { set_error("excenv_allgather: bad count %lld", (long long)count_per_rank); return EXCENV_EINVAL; }
  if (!nccl_comm || ((!send || !recv) && count_per_rank > 0)) { set_error("excenv_allgather: NULL argument"); return EXCENV_ENULL; }
  if (count_per_rank == 0) return EXCENV_OK;
  const char* why = nullptr;
  nccl_allgather_fn fn = resolve_allgather(&why);
  if (!fn) { set_error("excenv_allgather: %s", why ? why : "RCCL unavailable"); return EXCENV_EUNSUPPORTED; }
  const int nccl_type = dtype == EXCENV_F32 ? 7 : 8;  // ncclFloat32 / ncclFloat64 (rccl.h)
  const int rc = fn(send, recv, (size_t)count_per_rank, nccl_type, nccl_comm, (hipStream_t)stream);
  if (rc != 0) { set_error("excenv_allgather: ncclAllGather failed with ncclResult_t %d", rc); return EXCENV_EHIP; }
  return EXCENV_OK;
}

int excenv_probe_math(int which, int dtype, int64_t n, const void* in, void* out, void* stream) {
  if (which < 0 || which > 4 || n < 0 || (dtype != EXCENV_F32 && dtype != EXCENV_F64)) { set_error("excenv_probe_math: bad argument"); return EXCENV_EINVAL; }
  if (which > 2 && dtype != EXCENV_F64) { set_error("excenv_probe_math: which = 3 / 4 (sincos_lean) exist in fp64 only"); return EXCENV_EINVAL; }
  if (!in || !out) { set_error("excenv_probe_math: NULL argument"); return EXCENV_ENULL; }
  if (n == 0) return EXCENV_OK;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (dtype == EXCENV_F32)
    hipLaunchKernelGGL((probe_kernel<float>), grid, block, 0, (hipStream_t)stream, which, n, (const float*)in, (float*)out);
  else
    hipLaunchKernelGGL((probe_kernel<double>), grid, block, 0, (hipStream_t)stream, which, n, (const double*)in, (double*)out);
  return check_launch("excenv_probe_math");
}

int excenv_probe_div(int dtype, int64_t n, const void* num, const void* den, void* out_fast, void* out_ref, void* stream) {
  if (n < 0 || (dtype != EXCENV_F32 && dtype != EXCENV_F64)) { set_error("excenv_probe_div: bad argument"); return EXCENV_EINVAL; }
  if (!num || !den || !out_fast || !out_ref) { set_error("excenv_probe_div: NULL argument"); return EXCENV_ENULL; }
  if (n == 0) return EXCENV_OK;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (dtype == EXCENV_F32)
    hipLaunchKernelGGL((probe_div_kernel<float>), grid, block, 0, (hipStream_t)stream, n, (const float*)num, (const float*)den,
                       (float*)out_fast, (float*)out_ref);
  else
    hipLaunchKernelGGL((probe_div_kernel<double>), grid, block, 0, (hipStream_t)stream, n, (const double*)num,
                       (const double*)den, (double*)out_fast, (double*)out_ref);
  return check_launch("excenv_probe_div");
}

}  // extern "C"
