/*
 * excenv.h — C ABI of the MI355X-native batched ODE stepper behind
 * exciting-environments' vmap_step / vmap_sim_ahead hot path.
 *
 * The reference has no FFI of its own (it is pure Python on JAX/diffrax); the
 * boundary it exposes is the object returned by EnvironmentRegistry.X.make()
 * (reference exciting_environments/registration.py:21-32). Each entry point below
 * names the reference method whose arithmetic it replaces. All pointers are raw
 * device pointers (hipMalloc'ed / torch CUDA storage), sizes are plain integers,
 * `stream` is a hipStream_t passed as void*. No function throws, allocates device
 * memory, or synchronises the device: they only enqueue kernels on `stream`
 * (hipGraph-capturable). Return value: 0 on success, a negative EXCENV_E* code
 * otherwise; excenv_last_error() gives the per-thread message.
 *
 * Data layout (struct-of-arrays): every state field / per-env parameter is its
 * own contiguous [B] array. Trajectories come in three layouts:
 *   EXCENV_LAYOUT_ENV_MAJOR  : element (b,k,c) at ((b*K)+k)*C + c  — the reference's
 *                              row-major jnp arrays actions[B,K,A], observations[B,K+1,O],
 *                              state leaves [B,K+1] (core_env.py:571-616).
 *   EXCENV_LAYOUT_LANE_MAJOR : element (b,k,c) at ((k*C)+c)*B + b  — one lane per env,
 *                              lane-adjacent envs address-adjacent (fully coalesced).
 *   EXCENV_LAYOUT_TILED      : lane-major inside tiles of EXCENV_TILE envs: element (b,k,c) at
 *                              (b/TILE)*K*C*TILE + ((k*C)+c)*TILE + b%TILE — every workgroup owns one tile and
 *                              writes ONE sequential stream (fp32, batch_size % TILE == 0, unbatched properties).
 */
#ifndef EXCENV_H
#define EXCENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: v3 + excenv_random_state, excenv_update_ref_to, excenv_observe (additions only; every v3 signature is unchanged)
 * 5: v4 + excenv_stream_pattern (addition only)
 * 6: v5 + excenv_launch_opts_t.flags (the former `reserved` field; 0 keeps the old meaning); excenv_sim_ahead reads row-major
 *    actions inside the lane-major trajectory kernel (no workspace needed for that combination); additions:
 *    excenv_sim_ahead_fuses_actions, excenv_last_launch, excenv_allgather
 * 7: the lane-major truncated-flag trajectory is [row][B][flag] (an environment's flags adjacent; was [row][flag][B]):
 *    excenv_traj_gym_t.truncated of excenv_sim_ahead and the `truncated` output of excenv_rew_trunc_term. Every signature
 *    is unchanged; the env-major layout [B][row][flag] — the reference's — is untouched
 *    (still 7: EXCENV_OPT_KEEP_CONSTANT_COLUMNS, a flag bit older callers never set) */
#define EXCENV_ABI_VERSION 7

/* Environment ids. Field orders follow the reference dataclasses. */
typedef enum {
  EXCENV_PENDULUM = 0,           /* pendulum/pendulum_env.py:116-142   S=(theta,omega) A=(torque) P=(g,l,m) */
  EXCENV_MASS_SPRING_DAMPER = 1, /* mass_spring_damper_env.py:113-139  S=(deflection,velocity) A=(force) P=(d,k,m) */
  EXCENV_CART_POLE = 2,          /* cart_pole_env.py:126-157           S=(deflection,velocity,theta,omega) A=(force) P=(mu_p,mu_c,l,m_p,m_c,g) */
  EXCENV_ACROBOT = 3,            /* acrobot_env.py:135-169             S=(theta_1,theta_2,omega_1,omega_2) A=(torque) P=(g,l_1,l_2,m_1,m_2,l_c1,l_c2,I_1,I_2) */
  EXCENV_FLUID_TANK = 4,         /* fluid_tank_env.py:70-95            S=(height) A=(inflow) P=(base_area,orifice_area,c_d,g) */
  EXCENV_PMSM = 5,               /* pmsm/pmsm_env.py:269-305 (linear dq model) S=(u_d_buffer,u_q_buffer,epsilon,i_d,i_q,torque,omega_el)
                                    A=(u_d,u_q) P=(p,r_s,l_d,l_q,psi_p,u_dc,deadtime) O=(i_d,i_q,omega_el,torque,cos eps,sin eps,u_d_buffer,u_q_buffer) */
  EXCENV_NUM_ENVS = 6
} excenv_env_t;

/* Fixed-step explicit solvers (stand-ins for diffrax.Euler / diffrax.Tsit5 passed as
 * `solver=`; RK4 is a build-side extension). */
typedef enum { EXCENV_EULER = 0, EXCENV_RK4 = 1, EXCENV_TSIT5 = 2, EXCENV_NUM_SOLVERS = 3 } excenv_solver_t;

typedef enum { EXCENV_F32 = 0, EXCENV_F64 = 1 } excenv_dtype_t;

typedef enum { EXCENV_LAYOUT_ENV_MAJOR = 0, EXCENV_LAYOUT_LANE_MAJOR = 1, EXCENV_LAYOUT_TILED = 2 } excenv_layout_t;
#define EXCENV_TILE 1024 /* environments per tile of EXCENV_LAYOUT_TILED */

/* Trajectory semantics of excenv_sim_ahead.
 *   EXCENV_SEM_STEP  : the K steps are exactly K applications of excenv_step (post-processing —
 *                      angle wrap, tank clip, PMSM angle prediction — acts on the carried state).
 *                      This is the property the reference tests (tests/envs/test_core_functions.py:134-155).
 *   EXCENV_SEM_AHEAD : structure of the reference's _ode_solver_simulate_ahead (e.g.
 *                      pendulum_env.py:196-259, fluid_tank_env.py:156-216, pmsm_env.py:709-801): the raw
 *                      ODE state is carried un-wrapped / un-clipped, post-processing is applied to the SAVED
 *                      rows only, PMSM clips all actions with the predicted angle eps0 + k*tau*omega, and RK
 *                      stages with c_i == 1 read action k+1 (core_env.py:435-439). Step size is exactly
 *                      obs_stepsize and the action index is exactly floor(step / substeps): the documented
 *                      contract, and the default of the Python API.
 *   EXCENV_SEM_AHEAD_ACCUMULATED_T : opt-in; EXCENV_SEM_AHEAD on diffrax's accumulated-time clock as the CPU
 *                      oracle restates it (unpinned: not checked against diffrax itself). (t_prev, t_next) are
 *                      carried in the working precision from (0, obs_stepsize); each solver step has the size
 *                      t_next - t_prev, then (t_prev, t_next) = (t_next, 2 t_next - t_prev) with t_next snapped to
 *                      t_end = obs_stepsize * substeps * K within 1e-6 (fp32) / 1e-10 (fp64). The first stage and
 *                      stages with 0 < c_i < 1 read action int(t_prev / (obs_stepsize * substeps)), stages with
 *                      c_i == 1 action int(t_next / (obs_stepsize * substeps)), both clamped to [0, K - 1] (the
 *                      reference's actions[int(t / action_stepsize)], pendulum_env.py:215-216). In fp32 the row
 *                      differs from EXCENV_SEM_AHEAD's in most steps of a typical chunk. Known limit: literal
 *                      diffrax evaluates stages with 0 < c_i < 1 at t_prev + c_i * dt (RK4 / Tsit5 only). K must be
 *                      below 2^30. A library older than this value rejects it with EXCENV_EINVAL (same ABI version).
 */
typedef enum { EXCENV_SEM_STEP = 0, EXCENV_SEM_AHEAD = 1, EXCENV_SEM_AHEAD_ACCUMULATED_T = 2 } excenv_semantics_t;

#define EXCENV_MAX_STATE 8
#define EXCENV_MAX_ACTION 2
#define EXCENV_MAX_STATIC 9
#define EXCENV_MAX_CONTROL 8

/* A property leaf is either broadcast (per_env == NULL, `value` used) or batched
 * (per_env -> [B] array of the working dtype): reference core_env.py:253-277. */
typedef struct {
  double value;
  const void* per_env;
} excenv_param_t;

/* PMSM saturated model (pmsm_env.py:316-363, 487-507): the six look-up tables of the flux linkages / differential
 * inductances over the (i_d, i_q) grid, prepared as the reference's generate_interpolators_and_lut does (NaNs filled
 * by nearest neighbour, edges repeated once). All arrays are device arrays of the working dtype.
 *   grid_d [n_d], grid_q [n_q] : strictly increasing grid coordinates
 *   tables [n_d][n_q][8]       : (L_dd, L_dq, L_qd, L_qq, Psi_d, Psi_q, 0, 0) at each grid node */
typedef struct {
  int32_t n_d, n_q;
  const void* grid_d;
  const void* grid_q;
  const void* tables;
} excenv_pmsm_lut_t;

/* EnvProperties (core_env.py:245-251): static params in the field order listed at the env id,
 * min/max of physical_normalizations per state field and of action_normalizations per action.
 * pmsm_lut: NULL, or (EXCENV_PMSM only) the LUTs of the saturated model — selects nonlinear_ode /
 * currents_to_torque_saturated instead of the linear dq model (EnvProperties.saturated, pmsm_env.py:307-314). */
typedef struct {
  excenv_param_t static_params[EXCENV_MAX_STATIC];
  excenv_param_t state_min[EXCENV_MAX_STATE];
  excenv_param_t state_max[EXCENV_MAX_STATE];
  excenv_param_t action_min[EXCENV_MAX_ACTION];
  excenv_param_t action_max[EXCENV_MAX_ACTION];
  const excenv_pmsm_lut_t* pmsm_lut;
} excenv_props_t;

/* Reference-tracking columns of the observation (generate_observation appends the normalised
 * `state.reference.<name>` for every name in control_state, e.g. pendulum_env.py:322-328).
 * n_control == 0 => no extra columns. reference[j] is a [B] array for state field control_idx[j]. */
typedef struct {
  int32_t n_control;
  int32_t control_idx[EXCENV_MAX_CONTROL];
  const void* reference[EXCENV_MAX_CONTROL];
  /* excenv_gym_step only: NULL, or the [B] reference values the OBSERVATION columns show when they differ from the ones the
   * reward is computed against — GymWrapper.gym_step takes the observation before update_ref and the reward after it
   * (gym_wrapper.py:109-126), so in a step that redraws a reference the two differ. */
  const void* obs_reference[EXCENV_MAX_CONTROL];
} excenv_control_t;

/* Per-call launch options (no reference counterpart; NULL = all defaults). Everything that shapes a launch travels
 * with the call: the library keeps no mutable state besides the per-thread error string.
 *   envs_per_lane  : lane-major / tiled trajectories and the step path: 0 = auto (16-byte accesses when the batch is large
 *                    enough to fill the chip that way, else one env per lane), 1 / 2 / 4 = forced. Ignored (always 1) by
 *                    excenv_gym_step and by every call that needs the general instantiation (per-env property arrays,
 *                    gym trajectories, row-major buffers)
 *   env_major_mode : env-major (row-major) buffers — 0: a fused kernel when both layouts are env-major and substeps == 1
 *                    (the register-ring form for large batches of broadcast-property environments with 128-byte aligned
 *                    trajectory arrays, else the LDS-ring form); 1: never (workspace + transposes, or generic strides);
 *                    2: fused, LDS-ring form only; 3: fused, register-ring form whenever its preconditions hold
 *   lds_pad_bytes  : extra dynamic LDS per sim_ahead workgroup (caps resident workgroups per CU; occupancy experiments)
 *   flags          : bit set of EXCENV_OPT_* (0 = defaults; unknown bits are an error)
 *     EXCENV_OPT_NO_FUSED_ACTIONS : row-major actions with lane-major trajectories are transposed through the workspace
 *                                   (or read with generic strides) instead of being read by the trajectory kernel itself
 *     EXCENV_OPT_KEEP_CONSTANT_COLUMNS : excenv_sim_ahead[_ws] only. The caller guarantees that in the lane-major output buffers
 *                                   of this call every row of a time-constant column equals that column's row 0, for every
 *                                   environment — true of buffers an earlier excenv_sim_ahead call of the same shape and layout
 *                                   has written and nothing has modified since. PMSM (no look-up tables): omega_el is a constant
 *                                   of a trajectory, so a wave whose environments all find row 0 of the omega_el state leaf and
 *                                   of observation column 2 bit-equal to what it is about to store there leaves both columns
 *                                   alone (8 of the 68 bytes per environment-step in fp32); a wave in which any environment
 *                                   differs writes everything. Results are the same bits either way. Takes no part in choosing
 *                                   the kernel form; ignored by every other model and by every form but the lean lane-major one
 *                                   (per-environment properties, control columns written by the kernel, row-major actions read
 *                                   by the kernel, env-major and tiled trajectories, trajectories that go through a workspace) */
#define EXCENV_OPT_NO_FUSED_ACTIONS 1
#define EXCENV_OPT_KEEP_CONSTANT_COLUMNS 2
typedef struct {
  int32_t envs_per_lane;
  int32_t env_major_mode;
  int32_t lds_pad_bytes;
  int32_t flags; /* ABI <= 5: `reserved`, had to be 0 */
} excenv_launch_opts_t;

/* Optional reward / terminated / truncated trajectories of excenv_sim_ahead — what
 * CoreEnvironment.vmap_generate_rew_trunc_term_ahead (core_env.py:490-531, 618-647) computes from the returned states,
 * produced by the same launch from the registers that hold each saved state. All three pointers or NULL struct.
 *   reward     : N rows (saved rows 1..N) of one value per env, working dtype
 *   terminated : N rows of one byte (0/1) per env
 *   truncated  : N+1 rows (saved rows 0..N) of excenv_truncated_width() bytes per env
 * in the trajectory layout of the call: env-major reward / terminated [B][row], truncated [B][row][flag]; lane-major reward /
 * terminated [row][B], truncated [row][B][flag] (the flags of an environment adjacent: a lane of the trajectory kernel writes
 * the flags of its environments with one or two stores per row). Tiled: unsupported. */
typedef struct {
  void* reward;
  uint8_t* terminated;
  uint8_t* truncated;
} excenv_traj_gym_t;

/* ---- introspection -------------------------------------------------------------------- */
int excenv_abi_version(void);
const char* excenv_last_error(void);
/* Name of the kernel form the last launching call of this thread enqueued ("" before the first). excenv_sim_ahead[_ws]:
 * "sim_ahead_kernel (V=1|V=2|V=4)", "sim_ahead_kernel (general)", "sim_ahead_kernel (row-major actions fused)",
 * "sim_ahead_emr_kernel", "sim_ahead_em_kernel[ (general)]", "transposition workspace + sim_ahead_kernel". excenv_step:
 * "step_kernel (V=1|V=2|V=4)" (a forced opts->envs_per_lane that the batch size or a state pointer off a 16-byte boundary does
 * not allow runs, and reports, a narrower form), "step_kernel (general)" (per-environment properties, control columns or gym
 * outputs). The reverse-mode calls name theirs below. Informational (tests assert that the path they mean to check is the one
 * that ran). */
const char* excenv_last_launch(void);
/* S = physical_state_dim, A = action_dim, O = observation width without control columns, P = #static params. */
int excenv_env_dims(int env, int32_t* S, int32_t* A, int32_t* O, int32_t* P);
/* Algorithmic HBM bytes per env-step: w*(S+A+S+O) for the step path,
 * w*(A+O[+S]) for sim_ahead. */
int64_t excenv_step_bytes(int env, int dtype);
int64_t excenv_sim_ahead_bytes(int env, int dtype, int with_state_traj);

/* ---- replaces CoreEnvironment.vmap_step (core_env.py:533-569) -------------------------
 * and, for PMSM, PMSM.step (pmsm_env.py:851-883).
 *   state_in  : S pointers to [B] arrays (physical_state fields, reference order)
 *   action    : [B][A] row-major normalised action
 *   state_out : S pointers to [B] arrays (may alias state_in element-for-element)
 *   obs       : [B][O + n_control] row-major
 */
int excenv_step(int env, int solver, int dtype, int64_t B,
                const excenv_props_t* props, const excenv_control_t* control, double tau,
                const void* const* state_in, const void* action,
                void* const* state_out, void* obs, const excenv_launch_opts_t* opts, void* stream);

/* ---- replaces GymWrapper.gym_step (gym_wrapper.py:88-130): vmap_step fused with the environment's
 * generate_reward / generate_terminated / generate_truncated (e.g. pendulum_env.py:297-309,381-390,
 * pmsm_env.py:972-1037) so the new state is not read a second time.
 *   reward     : [B] values of the working dtype (the reference's [B,1])
 *   terminated : [B] bytes (0/1)
 *   truncated  : [B][excenv_truncated_width(env, n_control)] bytes (0/1): |obs| > 1 per observation column; one flag
 *                for PMSM (|i_dq| > 1 in normalised units) and FluidTank (constant 0)
 * The reference-generator (update_ref / generate_new_ref, JAX Threefry) is not part of this entry point. */
int32_t excenv_truncated_width(int env, int32_t n_control);
int excenv_gym_step(int env, int solver, int dtype, int64_t B,
                    const excenv_props_t* props, const excenv_control_t* control, double tau,
                    const void* const* state_in, const void* action,
                    void* const* state_out, void* obs, void* reward, uint8_t* terminated, uint8_t* truncated,
                    const excenv_launch_opts_t* opts, void* stream);

/* ---- replaces CoreEnvironment.vmap_sim_ahead (core_env.py:571-616) --------------------
 * and PMSM.sim_ahead (pmsm_env.py:746-801). One persistent launch runs all N = K*substeps
 * solver steps of step size obs_stepsize; action k is held for `substeps` solver steps.
 *   actions    : K rows of A normalised actions per env, in `action_layout`
 *   obs_traj   : N+1 rows of (O + n_control) per env, in `traj_layout` (row 0 = init state)
 *   state_traj : NULL, or S pointers to [B][N+1] (env-major) / [N+1][B] (lane-major) arrays
 *   last_state : S pointers to [B] arrays (row N of the trajectory; may alias state_in)
 *   env_tau    : the environment's own tau; only PMSM reads it (its voltage-angle prediction uses
 *                self.tau, pmsm_env.py:599-604,719-722, while the solver steps by obs_stepsize).
 *                PMSM requires substeps == 1 (reference quirk, pmsm_env.py:787).
 */
int excenv_sim_ahead(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                     const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                     double env_tau, const void* const* state_in, const void* actions, int action_layout,
                     void* obs_traj, void* const* state_traj, int traj_layout,
                     void* const* last_state, int semantics, const excenv_traj_gym_t* gym,
                     const excenv_launch_opts_t* opts, void* stream);

/* Same as excenv_sim_ahead, with a caller-provided device workspace. When a layout is EXCENV_LAYOUT_ENV_MAJOR
 * (the reference's row-major arrays) and `workspace_bytes >= excenv_sim_ahead_workspace_bytes(...)`, the library
 * transposes the actions into the workspace, runs the coalesced lane-major kernel there and transposes the
 * trajectories back with an LDS-tiled kernel (3 launches + S small ones, all on `stream`); without a workspace the
 * generic-stride path of the same kernel is used (one lane per env, scattered words). Results are bit-identical. */
int64_t excenv_sim_ahead_workspace_bytes(int env, int dtype, int64_t B, int64_t K, int32_t substeps, int32_t n_control,
                                         int action_layout, int traj_layout, int with_state_traj);
int excenv_sim_ahead_ws(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                        const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                        double env_tau, const void* const* state_in, const void* actions, int action_layout,
                        void* obs_traj, void* const* state_traj, int traj_layout, void* const* last_state,
                        int semantics, const excenv_traj_gym_t* gym, void* workspace, int64_t workspace_bytes,
                        const excenv_launch_opts_t* opts, void* stream);
/* 1 when excenv_sim_ahead[_ws] with these arguments reads the row-major actions[B][K][A] (what the reference's
 * vmap_sim_ahead is handed, core_env.py:571-616) inside the lane-major trajectory kernel itself — 64-byte windows of every
 * environment's row through LDS, no transposition pass, no workspace — else 0 (then a workspace of
 * excenv_sim_ahead_workspace_bytes lets the library transpose them first). Applies to broadcast properties without gym
 * trajectories (control columns are filled by a second small launch behind the lean kernel), the batch sizes that run
 * V = 16 / sizeof(dtype) environments per lane with B % (64 V) == 0, K * A * sizeof(dtype) a multiple of 16 and 16-byte aligned
 * actions. The answer assumes what the query cannot see: every control->reference[j] non-NULL, and the state_in, last_state,
 * state_traj and obs_traj arrays 16-byte aligned (as for every vectorised launch). It describes EXCENV_SEM_STEP and
 * EXCENV_SEM_AHEAD calls: under EXCENV_SEM_AHEAD_ACCUMULATED_T row-major actions are never fused. */
int excenv_sim_ahead_fuses_actions(int env, int solver, int dtype, int64_t B, int64_t K, const excenv_props_t* props,
                                   int32_t n_control, int with_gym, int action_layout, int traj_layout, const void* actions,
                                   const excenv_launch_opts_t* opts);
/* ---- reverse mode of excenv_sim_ahead (what jax.grad of the reference's vmap_sim_ahead gives; addition, same ABI version: a
 * binder probes for the symbol). One persistent launch computes the vector-Jacobian product of a trajectory call from the state
 * rows that call saved: it re-evaluates one step's stages per row and streams the rows from N down to 0.
 *   control         : only n_control is read (the width of a grad_obs_traj row; the control columns' cotangents are skipped:
 *                     those columns are constants of the trajectory)
 *   actions         : the forward call's actions, EXCENV_LAYOUT_LANE_MAJOR, or EXCENV_LAYOUT_ENV_MAJOR with a workspace of
 *                     excenv_sim_ahead_vjp_workspace_bytes (the library transposes them into it, excenv_transpose's kernel)
 *   state_traj      : S pointers to the lane-major [N+1][B] state trajectories the forward call wrote
 *   grad_obs_traj   : cotangent of obs_traj, lane-major [N+1][O + n_control][B], or NULL
 *   grad_state_traj : NULL, or S pointers to cotangents of the state trajectories ([N+1][B]), each may be NULL
 *   grad_last_state : NULL, or S pointers to cotangents of last_state ([B]), each may be NULL
 *   grad_actions    : out, lane-major [K][A][B]
 *   grad_state_in   : out, S pointers to [B]: the gradient w.r.t. every leaf of the initial physical state
 *   semantics       : EXCENV_SEM_AHEAD or EXCENV_SEM_STEP, the forward call's
 * opts->envs_per_lane: 0 = the forward's batch rule, 1 or 16 / sizeof(dtype) = forced (the wide form needs B % that == 0 and
 * 16-byte aligned arrays). Derivatives of clamps / clips are 0 on the boundary, of sign 0, of the tank's sqrt term 0 at h <= 0.
 * Not supported, rejected before any launch: the saturated PMSM (pmsm_lut), EXCENV_SEM_AHEAD_ACCUMULATED_T, the tiled layout and
 * per-environment property arrays (EXCENV_EUNSUPPORTED). Gradients w.r.t. the static parameters: excenv_sim_ahead_vjp_params below.
 * excenv_last_launch() then reports "sim_ahead_vjp_kernel (V=1|V=2|V=4)".
 * Workspace: excenv_sim_ahead_vjp_workspace_bytes_for (addition) is the size for a given call — the transposed actions and,
 * for the tank under EXCENV_SEM_AHEAD with RK4 / Tsit5, the raw levels [N+1][B] a pass in front of the reverse launch restores
 * (the saved rows hold max(h, 0); an RK stage state built from a clamped row is not the one the forward built from the raw level).
 * excenv_sim_ahead_vjp_workspace_bytes is the transposed actions' part alone: enough for every other call, and a call that needs
 * more fails with EXCENV_EINVAL and the size. */
int64_t excenv_sim_ahead_vjp_workspace_bytes(int env, int dtype, int64_t B, int64_t K, int action_layout);
int64_t excenv_sim_ahead_vjp_workspace_bytes_for(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                                                 int semantics, int action_layout);
int excenv_sim_ahead_vjp(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                         const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                         double env_tau, const void* actions, int action_layout, const void* const* state_traj,
                         const void* grad_obs_traj, const void* const* grad_state_traj,
                         const void* const* grad_last_state, void* grad_actions, void* const* grad_state_in,
                         int semantics, void* workspace, int64_t workspace_bytes, const excenv_launch_opts_t* opts,
                         void* stream);

/* ---- gradients w.r.t. the static parameters (what jax.grad of the reference's vmap_sim_ahead w.r.t.
 * env_properties.static_params gives; additions, same ABI version: a binder probes for the symbols).
 * excenv_sim_ahead_vjp_params is excenv_sim_ahead_vjp — same arguments, same rejections, and bit for bit the same grad_actions and
 * grad_state_in — whose one launch (the PGRAD instantiation of the reverse kernel) also accumulates, per environment, the
 * gradient w.r.t. every requested leaf of props->static_params:
 *   grad_params : EXCENV_MAX_STATIC entries, each a 16-byte aligned [B] array of the working dtype (out) or NULL = not wanted.
 *                 All NULL, a non-NULL entry beyond the model's parameter count or for an integer leaf (PMSM's p and deadtime):
 *                 EXCENV_EINVAL, naming the entry. The properties themselves stay broadcast values: the [B] outputs are the
 *                 per-environment terms of the batch gradient (excenv_param_grad_sum adds them up). A leaf the vector field never
 *                 reads (acrobot's l_2) gets exact zeros. PMSM's u_dc is visible only where the hexagon clip is active; the
 *                 normalisation bounds are not differentiated.
 * excenv_last_launch() then reports "sim_ahead_vjp_kernel (V=1|V=2|V=4, PGRAD)"; a forced opts->envs_per_lane without a PGRAD
 * form is EXCENV_EINVAL as for the plain call.
 * excenv_param_differentiable: 1 if static parameter `index` of `env` has a gradient, 0 if it is an integer leaf, -1 for a bad
 * env or index.
 * excenv_param_grad_sum: out[j] = sum over the batch of per_env_ptrs[j][0..B) for j < n <= EXCENV_MAX_STATIC (host array of device
 * pointers; out: n device elements of `dtype`). Two small launches, fp64 accumulation, no atomics: the same B gives the same bits
 * on every run. workspace: excenv_param_grad_sum_workspace_bytes(dtype, B, n) bytes of device memory, 8-byte aligned. */
int excenv_sim_ahead_vjp_params(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps,
                                const excenv_props_t* props, const excenv_control_t* control, double obs_stepsize,
                                double env_tau, const void* actions, int action_layout, const void* const* state_traj,
                                const void* grad_obs_traj, const void* const* grad_state_traj,
                                const void* const* grad_last_state, void* grad_actions, void* const* grad_state_in,
                                int semantics, void* workspace, int64_t workspace_bytes, const excenv_launch_opts_t* opts,
                                void* stream, void* const* grad_params);
int excenv_param_differentiable(int env, int index);
int64_t excenv_param_grad_sum_workspace_bytes(int dtype, int64_t B, int32_t n);
int excenv_param_grad_sum(int dtype, int64_t B, int32_t n, const void* const* per_env_ptrs, void* out, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* out[n][m] = in[m][n] for a row-major M x N matrix of the given dtype (the conversion kernel used above). */
int excenv_transpose(int dtype, int64_t M, int64_t N, const void* in, void* out, void* stream);

/* ---- replaces CoreEnvironment.vmap_generate_rew_trunc_term_ahead (core_env.py:490-531, 618-647) for a trajectory that
 * is already in memory (the fused form is the `gym` argument of excenv_sim_ahead): one thread per (env, row).
 *   state_traj : S pointers to [B x rows] arrays with element strides (state_env_stride, state_row_stride) — any layout
 *                excenv_sim_ahead writes (lane-major: (1, B); env-major: (rows, 1))
 *   control    : reference[j] is the base of the reference values of field control_idx[j]; ref_strides[2j], [2j+1] are its
 *                element strides (env, row) — (1, 0) for a reference that is constant along the trajectory; NULL = (1, 0)
 *   reward     : rows-1 values per env (rows 1..), terminated: rows-1 bytes, truncated: rows x excenv_truncated_width bytes,
 *                laid out as `out_layout` (EXCENV_LAYOUT_ENV_MAJOR [B][row][flag] or EXCENV_LAYOUT_LANE_MAJOR: reward / terminated
 *                [row][B], truncated [row][B][flag]) */
int excenv_rew_trunc_term(int env, int dtype, int64_t B, int64_t rows, const excenv_props_t* props,
                          const excenv_control_t* control, const int64_t* ref_strides, const void* const* state_traj,
                          int64_t state_env_stride, int64_t state_row_stride, void* reward, uint8_t* terminated,
                          uint8_t* truncated, int out_layout, void* stream);

/* ---- reverse mode of the reward above (what jax.grad gives through the reference's generate_reward; additions, same ABI
 * version: a binder probes for the symbols). The reward of row n depends on the state of row n only: one launch of
 * rew_vjp_kernel evaluates the transposed reward at every saved row and writes the cotangents of the state leaves the reward reads,
 * in the layout excenv_sim_ahead_vjp takes as grad_state_traj.
 * excenv_rew_reads (host only): reads[j] = 1 where the reward reads state leaf j, else 0 — the controlled fields; PMSM: i_d and
 * i_q when both are controlled, i_d, i_q and torque when torque is controlled, nothing otherwise. EXCENV_EINVAL for a bad env,
 * n_control or index, EXCENV_ENULL for a NULL array.
 * excenv_rew_vjp: props, control, ref_strides, state_traj and its two strides as for excenv_rew_trunc_term (state_traj[j] may
 * be NULL for a leaf that is not read; per-environment property arrays and the saturated PMSM are accepted, the reward does not
 * depend on the look-up tables), then
 *   grad_reward     : cotangent of the reward, rows-1 values per env (row n >= 1 at index n-1) with element strides
 *                     (grad_env_stride, grad_row_stride); may be NULL when rows == 1
 *   grad_state_traj : S pointers (out), lane-major [rows][B] each. Row 0 is written as zeros (the reward covers rows 1..). NULL for
 *                     a leaf that is read: EXCENV_ENULL, naming the leaf; a non-NULL array of a leaf that is not read is zero-filled.
 * Two forms with the same bits; excenv_last_launch() names the one that ran: "rew_vjp_kernel (V=2|V=4)", 16 bytes per lane, when
 * the state leaves are lane-major (strides (1, B)), B % (16 / sizeof(dtype)) == 0, every array is 16-byte aligned, each reference
 * is constant along rows (strides (1, 0)) or lane-major, grad_reward is lane-major and no property is a per-environment array;
 * "rew_vjp_kernel (V=1, strided)", one element per lane, otherwise. opts->envs_per_lane: 0 = that rule, 1 or 16 / sizeof(dtype) =
 * forced (a width that cannot be had: EXCENV_EINVAL). B == 0 returns EXCENV_OK without a launch, rows == 1 writes the zero row only.
 * Subgradients: the torque reward's derivative is that of the branch the forward selected (0 where none fired), |x| has derivative
 * sign(x) (0 at 0), sqrt(i_d^2 + i_q^2) has derivative 0 at the origin. References and normalisation bounds get no gradient. */
int excenv_rew_reads(int env, int32_t n_control, const int32_t* control_idx, uint8_t reads[EXCENV_MAX_STATE]);
int excenv_rew_vjp(int env, int dtype, int64_t B, int64_t rows, const excenv_props_t* props,
                   const excenv_control_t* control, const int64_t* ref_strides, const void* const* state_traj,
                   int64_t state_env_stride, int64_t state_row_stride, const void* grad_reward, int64_t grad_env_stride,
                   int64_t grad_row_stride, void* const* grad_state_traj, const excenv_launch_opts_t* opts, void* stream);

/* ---- reverse mode of ONE excenv_step / excenv_gym_step call (what jax.grad gives through the reference's vmap_step inside a closed
 * loop, where the action of step n is a function of the observation of step n; additions, same ABI version: a binder probes for the
 * symbols). One launch of step_vjp_kernel, one lane per environment, the arithmetic of a row of excenv_sim_ahead_vjp under
 * EXCENV_SEM_STEP with the transposed reward folded in:
 *   state_in, action  : what the forward call was handed (S x [B]; row-major [B][A], 16-byte aligned)
 *   state_out         : S x [B], the state the forward call returned. It is read as the post-processed state, not recomputed.
 *   grad_obs          : cotangent of obs, row-major [B][O + n_control] (control->n_control; 16-byte aligned), or NULL. The control
 *                       columns are skipped: references get no gradient.
 *   grad_state_out    : NULL, or S pointers ([B] or NULL each): cotangent of the returned state
 *   grad_reward       : cotangent of excenv_gym_step's reward, [B], or NULL. With it `control` carries the controlled fields and
 *                       their [B] references (control->reference; obs_reference is not read); without it only n_control is read.
 *   grad_state_in     : S x [B] (out), grad_action: row-major [B][A] (out, 16-byte aligned)
 * Never allocates or synchronises; graph-capturable. B == 0 returns EXCENV_OK without a launch. excenv_last_launch() names the
 * form: "step_vjp_kernel (V=1)", the only one (opts->envs_per_lane other than 0 or 1: EXCENV_EINVAL). EXCENV_ENULL names a missing
 * required pointer. EXCENV_EUNSUPPORTED: the saturated PMSM (pmsm_lut), per-environment property arrays, a grad_reward without
 * control references. Subgradient conventions as excenv_sim_ahead_vjp and excenv_rew_vjp.
 * excenv_step_vjp_bytes (host only): the algorithmic bytes per environment, w (2S + A) in, plus w (O + n_control) with grad_obs,
 * w S with a state cotangent, w (1 + n_control) with grad_reward, and w (S + A) out; -1 for a bad argument. */
int excenv_step_vjp(int env, int solver, int dtype, int64_t B, const excenv_props_t* props, const excenv_control_t* control,
                    double tau, const void* const* state_in, const void* action, const void* const* state_out,
                    const void* grad_obs, const void* const* grad_state_out, const void* grad_reward,
                    void* const* grad_state_in, void* grad_action, const excenv_launch_opts_t* opts, void* stream);
int64_t excenv_step_vjp_bytes(int env, int dtype, int32_t n_control, int has_grad_obs, int has_grad_state, int has_grad_reward);

/* ---- linearisation of excenv_step (what jax.jacobian gives through the reference's vmap_step): the Jacobians of `rows` stored
 * steps of B environments each from ONE launch of step_jac_kernel (additions, same ABI version: a binder probes for the symbols).
 * A step instance is (row n, environment i); its lane reads the step's two states and its action once and writes the Jacobian row
 * by row, each row the arithmetic of excenv_step_vjp for a one-hot cotangent:
 *   state_in, state_out : S pointers each; step n of leaf j starts at state_in[j][n * state_row_stride + i] and ends at
 *                         state_out[j][n * state_row_stride + i], the state the forward returned (read, not recomputed). A single
 *                         step has rows == 1; a lane-major state trajectory [N+1][B] passes state_out[j] = state_in[j] + B,
 *                         state_row_stride = B and rows = N.
 *   action              : element (action row k, component q, environment i) at k * action_row_stride + q * action_comp_stride +
 *                         i * action_env_stride elements. Step n reads action row n / substeps. Row-major [B][A]: (0, 1, A);
 *                         lane-major [K][A][B]: (A * B, B, 1). No alignment beyond the element's.
 *   dt, env_tau         : the solver's step (tau of excenv_step, obs_stepsize of excenv_sim_ahead) and the environment's tau
 *   row_kind            : EXCENV_JAC_STATE: R = S rows, row r = d new_state[r] / d (state, action);
 *                         EXCENV_JAC_OBS: R = O rows, row r = d obs[r] / d (state, action) at the saved new state. The n_control
 *                         reference columns of an observation are constants and have no rows; n_control is only validated.
 *   jacobian            : (out) lane-major [rows][R][S + A][B]: columns 0 .. S-1 the state leaves, S .. S+A-1 the action components
 * Never allocates or synchronises. B == 0 or rows == 0 returns EXCENV_OK without a launch. excenv_last_launch() names the form:
 * "step_jac_kernel (V=1, state rows)" or "step_jac_kernel (V=1, observation rows)" (opts->envs_per_lane other than 0 or 1:
 * EXCENV_EINVAL). EXCENV_ENULL names a missing pointer. EXCENV_EUNSUPPORTED: the saturated PMSM (pmsm_lut), per-environment
 * property arrays, PMSM with substeps != 1. Subgradient conventions as excenv_sim_ahead_vjp; static parameters, references and
 * bounds are not differentiated.
 * excenv_step_jacobian_bytes (host only): the algorithmic bytes per step instance, w (2S + A + R (S + A)); -1 for a bad argument. */
typedef enum { EXCENV_JAC_STATE = 0, EXCENV_JAC_OBS = 1 } excenv_jac_rows_t;
int excenv_step_jacobian(int env, int solver, int dtype, int64_t B, int64_t rows, int32_t substeps, const excenv_props_t* props,
                         int32_t n_control, double dt, double env_tau, const void* const* state_in, const void* const* state_out,
                         int64_t state_row_stride, const void* action, int64_t action_row_stride, int64_t action_comp_stride,
                         int64_t action_env_stride, int row_kind, void* jacobian, const excenv_launch_opts_t* opts, void* stream);
int64_t excenv_step_jacobian_bytes(int env, int dtype, int row_kind);

/* ---- closed-loop trajectories: excenv_sim_ahead under EXCENV_SEM_STEP with every action row computed INSIDE the one persistent
 * launch of sim_feedback_kernel, from the observation row saved at the action's start (an addition, same ABI version: a binder
 * probes for the symbol). Affine output feedback with optional integral action and a feedforward row. With N = K * substeps,
 * OW = O + n_control and obs_n the saved observation row n (reference columns included), at every action row k, n = k * substeps,
 * per environment and action component q:
 *   acc = ff[k][q] (0 without feedforward);  acc = acc + z[q] (with integral action only)
 *   acc = fma(gain[q][o], obs_n[o], acc) for o = 0 .. OW-1, in this order;  a[k][q] = min(max(acc, clip_lo), clip_hi)
 *   zi = 0;  zi = fma(integral_gain[q][o], obs_n[o], zi) for o = 0 .. OW-1
 *   z[q] = min(max(z[q] + action_stepsize * zi, clip_lo), clip_hi)            (action_stepsize = obs_stepsize * substeps)
 * and the normalised action a[k] is held for `substeps` steps of excenv_step's arithmetic (PMSM: hexagon constraint and dead-time
 * buffer included, substeps == 1). A NaN passes through both clamps; the integrator's clamp is the anti-windup.
 *   gain, integral_gain : lane-major [A][OW][gain_batch], gain_batch 1 (one gain set for every environment) or B (one per
 *                         environment); read once per launch
 *   feedforward         : lane-major [K][A][B] or NULL
 *   z_in, z_out         : the integrator state [A][B] before (NULL: zeros) and after the trajectory; both only touched with
 *                         integral_gain, which requires z_out. They may be the same array.
 *   obs_traj            : (out) [N+1][OW][B];  state_traj: (out) S pointers to [N+1][B], or NULL;  last_state: (out) S pointers to [B]
 *   actions_out         : (out) the applied normalised actions [K][A][B], or NULL
 * Rows are the post-processed states excenv_step carries: obs_traj / state_traj / last_state are bit for bit what excenv_sim_ahead
 * returns under EXCENV_SEM_STEP for `actions_out`. Properties may be per-environment arrays; pmsm_lut selects the saturated model
 * (tables read from global memory). Never allocates or synchronises. K == 0: row 0 only; B == 0: EXCENV_OK without a launch.
 * excenv_last_launch() reports "sim_feedback_kernel". EXCENV_ENULL names a missing pointer (policy, policy->gain, obs_traj,
 * last_state, z_out with integral_gain, ...). EXCENV_EINVAL: gain_batch other than 1 or B, clip_lo > clip_hi or a NaN bound, PMSM
 * with substeps != 1, opts->envs_per_lane other than 0 or 1 (one environment per lane is the only form). */
typedef struct {
  const void* gain;          /* [A][OW][gain_batch], required */
  const void* integral_gain; /* [A][OW][gain_batch] or NULL */
  int64_t gain_batch;        /* 1 or B */
  const void* feedforward;   /* [K][A][B] or NULL */
  const void* z_in;          /* [A][B] or NULL (zeros); read only with integral_gain */
  void* z_out;               /* [A][B]; required with integral_gain */
  double clip_lo;            /* -inf: no lower clamp */
  double clip_hi;            /* +inf: no upper clamp */
} excenv_feedback_t;
int excenv_sim_feedback(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                        const excenv_control_t* control, double obs_stepsize, double env_tau, const void* const* state_in,
                        const excenv_feedback_t* policy, void* obs_traj, void* const* state_traj, void* const* last_state,
                        void* actions_out, const excenv_launch_opts_t* opts, void* stream);

/* ---- policy rollouts: excenv_sim_feedback with a small multi-layer perceptron as the policy record, evaluated INSIDE the one
 * persistent launch of sim_policy_kernel (an addition, same ABI version: a binder probes for the symbol). Same EXCENV_SEM_STEP
 * rows, N = K * substeps, OW = O + n_control, obs_n = the saved observation row n (reference columns included). The network has
 * L = n_layers linear layers, 1 <= L <= EXCENV_POLICY_MAX_LAYERS, of widths d_0 = OW, d_1 .. d_{L-1} (hidden, each
 * 1 .. EXCENV_POLICY_MAX_WIDTH), d_L = A; L = 1 has no hidden layer. At every action row k, n = k * substeps, per environment:
 *   x^0 = obs_n
 *   for l = 1 .. L, for j = 0 .. d_l - 1:
 *     acc = b_l[j];  acc = fma(W_l[j][i], x^{l-1}[i], acc) for i = 0 .. d_{l-1} - 1, in this order
 *     x^l[j] = act(acc) for l < L, acc for l == L
 *   raw[q] = noise[k][q] + x^L[q]                  (one rounded add; without noise raw[q] = x^L[q], no add)
 *   a[k][q] = min(max(raw[q], clip_lo), clip_hi)   (a NaN passes through; -inf / +inf change nothing)
 * act is EXCENV_ACT_RELU, (acc < 0) ? 0 : acc, or EXCENV_ACT_TANH (within 5 ulp of tanh); one activation for all hidden layers.
 * The normalised action a[k] is held for `substeps` steps of excenv_step's arithmetic (PMSM: substeps == 1).
 *   params      : ONE device array shared by every environment, in the working dtype: for l = 1 .. L in turn W_l row-major
 *                 [d_l][d_{l-1}] (torch's nn.Linear.weight layout), then b_l [d_l]. Read-only, never copied or repacked.
 *   noise       : lane-major [K][A][B] (a pre-sampled exploration row per action) or NULL
 *   obs_traj    : (out) [N+1][OW][B];  state_traj: (out) S pointers to [N+1][B], or NULL;  last_state: (out) S pointers to [B]
 *   actions_out : (out) the applied normalised actions [K][A][B], or NULL
 * obs_traj / state_traj / last_state are bit for bit what excenv_sim_ahead returns under EXCENV_SEM_STEP for `actions_out`.
 * Properties may be per-environment arrays; pmsm_lut selects the saturated model. Never allocates or synchronises. K == 0: row 0
 * only; B == 0: EXCENV_OK without a launch. excenv_last_launch() reports "sim_policy_kernel". EXCENV_ENULL names a missing pointer
 * (policy, policy->params, obs_traj, last_state, a state pointer). EXCENV_EINVAL: n_layers outside 1 .. 4, a hidden width outside
 * 1 .. 64, widths[0] != OW or widths[L] != A, an unknown activation, clip_lo > clip_hi or a NaN bound, PMSM with substeps != 1,
 * opts->envs_per_lane other than 0 or 1. */
#define EXCENV_POLICY_MAX_LAYERS 4
#define EXCENV_POLICY_MAX_WIDTH 64
#define EXCENV_ACT_RELU 0
#define EXCENV_ACT_TANH 1
typedef struct {
  const void* params;                           /* W_1, b_1, .., W_L, b_L; required */
  int32_t n_layers;                             /* L */
  int32_t activation;                           /* EXCENV_ACT_RELU / EXCENV_ACT_TANH, of the hidden layers */
  int32_t widths[EXCENV_POLICY_MAX_LAYERS + 1]; /* d_0 .. d_L; entries past L are not read */
  const void* noise;                            /* [K][A][B] or NULL */
  double clip_lo;                               /* -inf: no lower clamp */
  double clip_hi;                               /* +inf: no upper clamp */
} excenv_policy_t;
int excenv_sim_policy(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                      const excenv_control_t* control, double obs_stepsize, double env_tau, const void* const* state_in,
                      const excenv_policy_t* policy, void* obs_traj, void* const* state_traj, void* const* last_state,
                      void* actions_out, const excenv_launch_opts_t* opts, void* stream);

/* ---- episode rollouts: excenv_sim_policy with rewards, flags and resets INSIDE the one persistent launch of
 * sim_episodes_kernel (an addition, same ABI version: a binder probes for the symbol). One solver step per action, as
 * GymWrapper.step does: substeps must be 1, so N = K. Per environment, with st_0 = state_in, t_0 = episode_steps_in (0 where NULL),
 * e = 0, R = n_reset_rows and TW = excenv_truncated_width(env, n_control):
 *   for n = 0 .. K:
 *     save row n: the observation row, the state row, truncated[n][:] = generate_truncated(st_n)
 *     if n >= 1: reward[n-1] = generate_reward(st_n), terminated[n-1] = generate_terminated(st_n)
 *     if n == K: break
 *     a[n] = clamp(noise[n] + mlp(obs row n))          (excenv_sim_policy's contract; written to actions_out[n] in every case)
 *     end_n = (end_mask & EXCENV_END_TERMINATED and terminated(st_n)) or (end_mask & EXCENV_END_TRUNCATED and any truncated(st_n)[:])
 *             or (max_episode_steps > 0 and t_n >= max_episode_steps)
 *     reset[n] = end_n
 *     if end_n: st_{n+1} = reset_states[e mod R];  e += 1;  t_{n+1} = 0         (the action is ignored)
 *     else:     st_{n+1} = excenv_step(st_n, a[n]);          t_{n+1} = t_n + 1  (bit for bit)
 *   last_state = st_K;  n_resets = e;  episode_steps_out = t_K
 * Row 0 is judged like every other row: its `terminated` value has no output slot, reset[0] shows the verdict. Every gym output is a
 * pure function of the saved row it belongs to, reset rows included, so reward / terminated / truncated are bit for bit what
 * excenv_rew_trunc_term gives on state_traj. A trainer masks the transitions with reset[n] == 1: row n is the terminal observation,
 * row n + 1 the first of the next episode. References are constant along the call; a reset does not redraw them. A reset state that
 * is itself terminal resets again on the next step. Without a control block the reward of the five non-PMSM models is 0 and their
 * terminated flag is `reward == 0`: with EXCENV_END_TERMINATED every step is then a reset (the reference's semantics);
 * EXCENV_END_TRUNCATED alone is the usual choice there.
 *   reset_states      : S pointers, each lane-major [R][B]; an environment's e-th reset within the call takes row e mod R
 *   episode_steps_in  : [B] int32 or NULL (zeros): the steps already taken in the running episode
 *   reward            : (out) [K][B], working dtype;  terminated: (out) [K][B] bytes;  truncated: (out) [K+1][B][TW] bytes: the
 *                       lane-major layouts of excenv_traj_gym_t;  reset: (out) [K][B] bytes;  n_resets, episode_steps_out: (out)
 *                       [B] int32. Each output may be NULL.
 * K == 0: row 0 and truncated[0] are written, n_resets = 0, episode_steps_out = episode_steps_in. B == 0: EXCENV_OK without a launch.
 * excenv_last_launch() reports "sim_episodes_kernel". Validated in excenv_sim_policy's order, then this record. EXCENV_ENULL: a NULL
 * record, NULL reset_states or a NULL leaf in it. EXCENV_EINVAL: substeps != 1, n_reset_rows < 1, unknown bits in end_mask,
 * max_episode_steps < 0, and end_mask == 0 with max_episode_steps == 0 (nothing could end an episode: excenv_sim_policy is that). */
#define EXCENV_END_TERMINATED 1
#define EXCENV_END_TRUNCATED 2
typedef struct {
  const void* const* reset_states; /* S pointers to [n_reset_rows][B]; required */
  int32_t n_reset_rows;            /* R >= 1 */
  int32_t end_mask;                /* EXCENV_END_TERMINATED | EXCENV_END_TRUNCATED */
  int32_t max_episode_steps;       /* >= 0; 0: no time limit */
  const int32_t* episode_steps_in; /* [B] or NULL (zeros) */
  void* reward;                    /* (out) [K][B] or NULL */
  uint8_t* terminated;             /* (out) [K][B] or NULL */
  uint8_t* truncated;              /* (out) [K+1][B][TW] or NULL */
  uint8_t* reset;                  /* (out) [K][B] or NULL */
  int32_t* n_resets;               /* (out) [B] or NULL */
  int32_t* episode_steps_out;      /* (out) [B] or NULL */
} excenv_episode_t;
int excenv_sim_policy_episodes(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                               const excenv_control_t* control, double obs_stepsize, double env_tau, const void* const* state_in,
                               const excenv_policy_t* policy, void* obs_traj, void* const* state_traj, void* const* last_state,
                               void* actions_out, const excenv_episode_t* episode, const excenv_launch_opts_t* opts, void* stream);

/* ---- reverse mode of excenv_sim_feedback: the vector-Jacobian product of one closed-loop trajectory with respect to the initial
 * state, the gains, the feedforward rows and the initial integrator state, from the rows that call saved (additions, same ABI
 * version: a binder probes for the symbols). The forward, at action row k (n = k * substeps, ob = saved observation row n with all
 * OW = O + n_control columns, adt = obs_stepsize * substeps):
 *   acc_k = ff[k] + z_k + Gp ob;  a_k = clamp(acc_k);  zi_k = Gi ob;  z_{k+1} = clamp(z_k + adt zi_k);
 *   s_{n+1 .. n+substeps} = env_step(s, a_k)
 * The reverse pass walks the rows from N down to 0 and carries sb[S] (cotangent of the carried state), zb[A] (cotangent of z_{k+1},
 * starting from grad_z) and ab[A] (the action cotangent summed over the `substeps` steps that held a_k). Per solver step
 * n = N-1 .. 0:
 *   1. sb += observe^T(grad_obs[n+1]) + grad_states[n+1] at the saved row n+1 (row N also takes grad_last_state). The control columns
 *      of grad_obs are skipped: references get no gradient.
 *   2. the transposed step of excenv_step_vjp takes sb from row n+1 back to row n, and ab += its action gradient.
 *   3. if n is an action row (n = k * substeps):
 *        ab += grad_actions[k]
 *        pre[q]  = ab[q] where clip_lo < a_k[q] < clip_hi, else 0        (the stored applied action)
 *        zpre[q] = zb[q] where clip_lo < z_{k+1}[q] < clip_hi, else 0    (the recomputed integrator row)
 *        grad_ff[k][q] = pre[q];  grad_zi[k][q] = adt * zpre[q]
 *        obb[o] = sum_q Gp[q][o] pre[q] + Gi[q][o] grad_zi[k][q]  for o < O;  sb += observe^T(obb) at s_n
 *        zb[q] = pre[q] + zpre[q];  ab = 0
 *   4. after row 0: sb += observe^T(grad_obs[0]) + grad_states[0]; grad_state0 = sb, grad_z0 = zb.
 * grad_gain[q][o] = sum_k pre_k[q] ob_k[o] and grad_integral_gain[q][o] = sum_k grad_zi_k[q] ob_k[o] over all OW columns (the gains
 * on reference columns do get gradients), k ascending, per environment. A clamp has derivative 0 on and outside its bounds; a NaN
 * compares false, so its gradient is 0. The other subgradient conventions are excenv_sim_ahead_vjp's.
 * Launches, all on `stream`, in this order: feedback_z_rows_kernel (with integral_gain and K > 0 only: the forward's own recurrence
 * over the saved observation rows, z_1 .. z_K into the workspace; its last row equals the forward's z_out bit for bit),
 * sim_feedback_vjp_kernel (one environment per lane), feedback_gain_grad_kernel (one launch for the requested gain gradients) and, for
 * gain_batch == 1, the deterministic batch sum of excenv_param_grad_sum in chunks of EXCENV_MAX_STATIC entries. No atomics.
 *   gain, integral_gain, gain_batch, clip_lo, clip_hi : as the forward call's policy
 *   obs_traj, state_traj, actions, z_in : what the forward wrote ([N+1][OW][B], S x [N+1][B], [K][A][B]) and was given (z_in, NULL =
 *                         zeros: the pre-pass rebuilds the integrator rows from it). state_traj and obs_traj are required.
 *   grad_obs            : [N+1][OW][B] or NULL;  grad_states, grad_last_state: NULL, or S pointers ([N+1][B] / [B], or NULL each)
 *   grad_actions        : [K][A][B] or NULL (cotangent of actions_out);  grad_z: [A][B] or NULL (cotangent of z_out)
 *   grad_state0         : (out) S pointers to [B];  grad_ff: (out) [K][A][B], required;  grad_zi: (out) [K][A][B] and grad_z0: (out)
 *                         [A][B], both required with integral_gain
 *   grad_gain, grad_integral_gain : (out) [A][OW][gain_batch] or NULL = not wanted
 *   workspace           : excenv_sim_feedback_vjp_workspace_bytes(env, dtype, B, K, n_control, gain_batch, integral_gain != NULL)
 *                         bytes of device memory, 8-byte aligned (-1 for a bad argument)
 * Never allocates or synchronises. K == 0 handles row 0 only; B == 0 returns EXCENV_OK without a launch. excenv_last_launch() reports
 * "sim_feedback_vjp_kernel". EXCENV_ENULL names a missing required pointer. EXCENV_EINVAL: gain_batch other than 1 or B, clip_lo >
 * clip_hi or a NaN bound, PMSM with substeps != 1, opts->envs_per_lane other than 0 or 1, a workspace that is too small (with the
 * size). EXCENV_EUNSUPPORTED: the saturated PMSM (pmsm_lut), per-environment property arrays.
 * excenv_sim_feedback_vjp_bytes (host only): the algorithmic bytes per environment and action row of the whole sequence; -1 for a
 * bad argument. */
typedef struct {
  const void* gain;                    /* [A][OW][gain_batch], required */
  const void* integral_gain;           /* [A][OW][gain_batch] or NULL */
  int64_t gain_batch;                  /* 1 or B */
  double clip_lo;
  double clip_hi;
  const void* obs_traj;                /* [N+1][OW][B], required */
  const void* const* state_traj;       /* S x [N+1][B], required */
  const void* actions;                 /* [K][A][B]: the applied actions */
  const void* z_in;                    /* [A][B] or NULL (zeros) */
  const void* grad_obs;                /* [N+1][OW][B] or NULL */
  const void* const* grad_states;      /* NULL, or S pointers ([N+1][B] or NULL each) */
  const void* const* grad_last_state;  /* NULL, or S pointers ([B] or NULL each) */
  const void* grad_actions;            /* [K][A][B] or NULL */
  const void* grad_z;                  /* [A][B] or NULL */
  void* const* grad_state0;            /* S x [B] */
  void* grad_ff;                       /* [K][A][B] */
  void* grad_zi;                       /* [K][A][B], with integral_gain */
  void* grad_z0;                       /* [A][B], with integral_gain */
  void* grad_gain;                     /* [A][OW][gain_batch] or NULL */
  void* grad_integral_gain;            /* [A][OW][gain_batch] or NULL */
} excenv_feedback_vjp_t;
int64_t excenv_sim_feedback_vjp_workspace_bytes(int env, int dtype, int64_t B, int64_t K, int32_t n_control, int64_t gain_batch,
                                                int integral);
int64_t excenv_sim_feedback_vjp_bytes(int env, int dtype, int32_t n_control, int32_t substeps, int integral, int has_grad_obs,
                                      int has_grad_states, int has_grad_actions);
int excenv_sim_feedback_vjp(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                            const excenv_control_t* control, double obs_stepsize, double env_tau,
                            const excenv_feedback_vjp_t* call, void* workspace, int64_t workspace_bytes,
                            const excenv_launch_opts_t* opts, void* stream);

/* ---- reverse mode of excenv_sim_policy: the vector-Jacobian product of one policy rollout with respect to the initial state and the
 * pre-clamp output of the network at every action row, from the rows that call saved (additions, same ABI version: a binder probes
 * for the symbols). The forward is excenv_sim_policy's contract. ONE launch of sim_policy_vjp_kernel, one environment per lane; it
 * has no cross-lane reduction and computes NO parameter gradient: with obs_k the saved observation row of action row k,
 *   grad_params = sum over b, k of (d mlp / d params)(obs[b][k])^T grad_raw[b][k],
 * a contraction over B * K independent samples that the caller does with its own BLAS on the rows the forward saved.
 * The reverse pass walks the rows from N down to 0 and carries sb[S] (cotangent of the carried state) and ab[A] (the action cotangent
 * summed over the `substeps` steps that held a_k), exactly as excenv_sim_feedback_vjp does. Per solver step n = N-1 .. 0:
 *   1. sb += observe^T(grad_obs[n+1]) + grad_states[n+1] at the saved row n+1 (row N also takes grad_last_state). The control columns
 *      of grad_obs are skipped: references get no gradient.
 *   2. the transposed step of excenv_step_vjp takes sb from row n+1 back to row n, and ab += its action gradient.
 *   3. if n is an action row (n = k * substeps):
 *        ab += grad_actions[k]
 *        pre[q] = ab[q] where clip_lo < a_k[q] < clip_hi (the stored applied action), else 0;   ab = 0
 *        grad_raw[k] = pre                     (= the cotangent of noise[k] and of the network output x^L)
 *        x^0 .. x^{L-1}: the forward's statements again on the STORED observation row n (all OW columns), every layer kept
 *        d^L = pre
 *        for l = L .. 1:  xb[i] = 0;  xb[i] = fma(W_l[j][i], d^l[j], xb[i]) for j = 0 .. d_l - 1, in this order
 *                         (for l = 1 only i < O: reference columns get no gradient)
 *                         d^{l-1}[i] = xb[i] * act'(x^{l-1}[i])   for l > 1
 *        sb += observe^T(xb of layer 1) at s_n
 *   4. after row 0: sb += observe^T(grad_obs[0]) + grad_states[0]; grad_state0 = sb.
 * act' is taken from the recomputed activation value h = x^{l-1}[i]: EXCENV_ACT_RELU passes xb where h > 0 and gives 0 elsewhere
 * (torch's convention; a NaN gets 0), EXCENV_ACT_TANH multiplies by 1 - h * h (a rounded product, then a rounded difference). The
 * clamp has derivative 0 on and outside its bounds; a NaN compares false, so its gradient is 0. The other subgradient conventions
 * are excenv_sim_ahead_vjp's.
 * Episode mask (optional, substeps == 1): reset is what excenv_sim_policy_episodes wrote. Where reset[n] != 0, step n -> n+1 was a
 * reset: the transposed step is skipped and what was accumulated for row n+1 is dropped (sb = 0: reset states get no gradient), and
 * ab holds grad_actions[n] only (the action was written but not applied). Step 3 then runs as usual.
 *   control             : only n_control is read (the reference columns come from the stored observation rows)
 *   policy              : the excenv_policy_t of the forward; `noise` is not read
 *   obs_traj, state_traj, actions : what the forward wrote ([N+1][OW][B], S x [N+1][B], [K][A][B]); all three are required
 *                         (actions with K > 0)
 *   reset               : [K][B] bytes or NULL
 *   grad_obs            : [N+1][OW][B] or NULL;  grad_states, grad_last_state: NULL, or S pointers ([N+1][B] / [B], or NULL each)
 *   grad_actions        : [K][A][B] or NULL (cotangent of actions_out)
 *   grad_state0         : (out) S pointers to [B];  grad_raw: (out) [K][A][B]; both required (grad_raw with K > 0)
 * Needs no workspace; never allocates or synchronises. K == 0 handles row 0 only; B == 0 returns EXCENV_OK without a launch.
 * excenv_last_launch() reports "sim_policy_vjp_kernel". Validated before any HIP call in excenv_sim_policy's order under this entry's
 * name (a NULL `call` first of all), then this record: EXCENV_ENULL names a missing required pointer; EXCENV_EINVAL: reset with
 * substeps != 1, K * substeps >= 2^31. EXCENV_EUNSUPPORTED: the saturated PMSM (pmsm_lut), per-environment property arrays.
 * excenv_sim_policy_vjp_bytes (host only): the algorithmic bytes per environment and action row: w * (substeps * (S + O [grad_obs] +
 * S [grad_states]) + OW + A * (2 + [grad_actions])) + [reset]; -1 for a bad argument. */
typedef struct {
  excenv_policy_t policy;              /* the forward's record; noise is not read */
  const void* obs_traj;                /* [N+1][OW][B], required */
  const void* const* state_traj;       /* S x [N+1][B], required */
  const void* actions;                 /* [K][A][B]: the applied actions */
  const uint8_t* reset;                /* [K][B] or NULL; needs substeps == 1 */
  const void* grad_obs;                /* [N+1][OW][B] or NULL */
  const void* const* grad_states;      /* NULL, or S pointers ([N+1][B] or NULL each) */
  const void* const* grad_last_state;  /* NULL, or S pointers ([B] or NULL each) */
  const void* grad_actions;            /* [K][A][B] or NULL */
  void* const* grad_state0;            /* (out) S x [B] */
  void* grad_raw;                      /* (out) [K][A][B] */
} excenv_policy_vjp_t;
int64_t excenv_sim_policy_vjp_bytes(int env, int dtype, int32_t n_control, int32_t substeps, int has_grad_obs, int has_grad_states,
                                    int has_grad_actions, int has_reset);
int excenv_sim_policy_vjp(int env, int solver, int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_props_t* props,
                          const excenv_control_t* control, double obs_stepsize, double env_tau, const excenv_policy_vjp_t* call,
                          const excenv_launch_opts_t* opts, void* stream);

/* ---- the parameter gradient of a policy rollout: the contraction excenv_sim_policy_vjp leaves to its caller, on the matrix cores
 * (additions, same ABI version: a binder probes for the symbols). It needs no environment, solver or properties, only the network
 * and two lane-major arrays:
 *   grad_params = sum over b < B, k < K of (d mlp / d params)(obs_traj[k * substeps][.][b])^T grad_raw[k][.][b]
 * with mlp the network of excenv_sim_policy and the derivative conventions of excenv_sim_policy_vjp: the hidden layers are evaluated
 * again (bias first, then the inputs in ascending order); EXCENV_ACT_RELU passes where the recomputed activation h > 0 and gives 0
 * elsewhere, EXCENV_ACT_TANH multiplies by 1 - h * h. All OW columns are read: the weights on reference columns get gradients. An
 * episode mask needs no handling: grad_raw already carries it.
 * Two launches on `stream`: policy_param_grad_kernel, then policy_param_grad_reduce_kernel. A sample tile is 64 consecutive
 * environments of one action row, tile number k * ceil(B / 64) + b_tile; with T tiles and G = min(T, max_groups > 0 ? max_groups :
 * EXCENV_PARAM_GRAD_AUTO_GROUPS) workgroups, workgroup g owns the tiles first(g) .. first(g + 1) - 1, first(g) = g * (T / G) +
 * min(g, T mod G): a function of (B, K, max_groups) only, never of the device, so the same call gives the same bits on every run. A
 * workgroup sums at most
 * EXCENV_PARAM_GRAD_CHAIN samples in the working dtype (v_mfma_*_16x16x4 accumulators: a k-ordered fused multiply-add chain) before
 * it adds them into its own fp64 slot of the workspace; the second launch adds the G slots of every parameter in ascending order in
 * fp64 and stores the working dtype. No atomics.
 *   policy      : params, n_layers, activation and widths of the forward; noise and the clip bounds are not read. widths[0] = OW is
 *                 1 .. EXCENV_POLICY_MAX_INPUT, widths[n_layers] = A is 1 .. EXCENV_MAX_ACTION
 *   obs_traj    : [K * substeps + 1][OW][B]: rows k * substeps are read;  grad_raw: [K][A][B], what excenv_sim_policy_vjp wrote
 *   grad_params : (out) [policy parameter count] of the working dtype, laid out like params: W_1, b_1, .., W_L, b_L
 *   workspace   : excenv_policy_param_grad_workspace_bytes(dtype, B, K, &policy, max_groups) bytes of device memory (G * parameter
 *                 count * 8; -1 for a bad argument), 8-byte aligned; needs no initialisation
 * Never allocates or synchronises. B == 0 returns EXCENV_OK without a launch; K == 0 with B > 0 writes zeros (the second launch
 * alone, over zero slots). excenv_last_launch() reports "policy_param_grad_kernel". Validated before any HIP call: EXCENV_ENULL names
 * a missing pointer (call, policy.params, obs_traj, grad_raw with K > 0, grad_params, workspace); EXCENV_EINVAL: dtype, B < 0, K < 0,
 * substeps < 1, K * substeps >= 2^31, n_layers outside 1 .. 4, a hidden width outside 1 .. 64, widths[0] outside 1 .. 16,
 * widths[n_layers] outside 1 .. 2, an unknown activation, max_groups < 0, a workspace that is too small or misaligned (with the
 * byte count). */
#define EXCENV_POLICY_MAX_INPUT 16        /* the widest observation row: 8 + EXCENV_MAX_CONTROL */
#define EXCENV_PARAM_GRAD_CHAIN 4096      /* samples one working-dtype accumulator sums before it goes to fp64 */
#define EXCENV_PARAM_GRAD_AUTO_GROUPS 512 /* workgroups of max_groups == 0, at most */
typedef struct {
  excenv_policy_t policy;   /* params, n_layers, activation, widths of the forward; noise and clip bounds are not read */
  const void* obs_traj;     /* [K * substeps + 1][OW][B], OW = widths[0]: rows k * substeps are read, all OW columns */
  const void* grad_raw;     /* [K][A][B], A = widths[n_layers]: what excenv_sim_policy_vjp wrote */
  void* grad_params;        /* (out) [policy parameter count] of the working dtype, laid out like params */
  void* workspace;          /* excenv_policy_param_grad_workspace_bytes bytes of device memory, 8-byte aligned; no initialisation */
  int64_t workspace_bytes;
  int32_t max_groups;       /* 0: auto; > 0: at most this many workgroups (tests, reproducibility across shapes) */
} excenv_policy_param_grad_t;
int64_t excenv_policy_param_grad_workspace_bytes(int dtype, int64_t B, int64_t K, const excenv_policy_t* policy, int32_t max_groups);
int excenv_policy_param_grad(int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_policy_param_grad_t* call, void* stream);

/* ---- the network of excenv_sim_policy on stored observation rows: the forward half beside
 * excenv_policy_param_grad, for the new means and the critic's values of an on-policy update. Model-free, lane-major:
 *   out[r][q][b] = x^L[q] of mlp(obs_traj[r * row_stride][.][b]),   r < R, q < A, b < B
 * with mlp excenv_sim_policy's network exactly: every unit starts at its bias and adds the inputs in ascending order, one fused
 * multiply-add each; EXCENV_ACT_RELU / EXCENV_ACT_TANH (the rollout's own functions) behind every layer but the last; no noise and no
 * clamp. out[r] is bit for bit the x^L sim_policy_kernel / sim_episodes_kernel computed for the same stored row, in fp32 and fp64 (the
 * stored row, reference columns included, is what the rollout's network read), so clamp(noise[k] + out[k]) reproduces actions_out[k].
 * One launch of policy_eval_kernel on `stream`. A sample tile is 64 consecutive environments of one evaluated row, tile number
 * r * ceil(B / 64) + b_tile; with T tiles and G = min(T, 2048) workgroups, workgroup g owns the tiles first(g) .. first(g + 1) - 1,
 * first(g) = g * (T / G) + min(g, T mod G): a function of (B, R) only.
 *   policy   : params, n_layers, activation and widths; noise and the clip bounds are not read. widths[0] = OW is
 *              1 .. EXCENV_POLICY_MAX_INPUT, widths[n_layers] = A is 1 .. EXCENV_MAX_ACTION. A critic is a network with A = 1.
 *   obs_traj : [(R - 1) * row_stride + 1 or more][OW][B]: rows r * row_stride are read, all OW columns
 *   out      : (out) [R][A][B] of the working dtype
 * Never allocates or synchronises. B == 0 or R == 0 returns EXCENV_OK without a launch. excenv_last_launch() reports
 * "policy_eval_kernel". Validated before any HIP call: EXCENV_ENULL names a missing pointer (call, policy.params, obs_traj, out);
 * EXCENV_EINVAL: dtype, B < 0, R < 0, row_stride < 1, (R - 1) * row_stride >= 2^31, n_layers outside 1 .. 4, a hidden width outside
 * 1 .. 64, widths[0] outside 1 .. 16, widths[n_layers] outside 1 .. 2, an unknown activation. */
typedef struct {
  excenv_policy_t policy;   /* params, n_layers, activation, widths; noise and clip bounds are not read */
  const void* obs_traj;     /* [(R - 1) * row_stride + 1 or more][OW][B], OW = widths[0]: rows r * row_stride are read */
  void* out;                /* (out) [R][A][B], A = widths[n_layers] */
} excenv_policy_eval_t;
int excenv_policy_eval(int dtype, int64_t B, int64_t R, int64_t row_stride, const excenv_policy_eval_t* call, void* stream);

/* ---- generalised advantage estimation on lane-major rows, in the convention of excenv_sim_policy_episodes:
 * reward[n] and terminated[n] belong to row n + 1; reset[n] says that row n is a terminal observation and row n + 1 the first one of
 * the next episode, so n -> n + 1 is no transition. An episode cut by `truncated` or by the step budget at row n + 1 has reset[n + 1]
 * set and bootstraps from value[n + 1], the terminal observation; a terminated episode does not bootstrap; row K bootstraps the
 * running episode. Arithmetic in the working dtype T with g = (T)gamma and gl = (T)(g * (T)lambda). Per environment, carry = 0; for
 * n = K - 1 down to 0:
 *   if reset[n]:  advantage[n] = 0;  returns[n] = value[n];  carry = 0      (not a transition: row n + 1 is a reset state)
 *   else:
 *       nt    = !terminated[n]
 *       boot  = nt ? value[n + 1] : 0                    (a select, not a product: a NaN behind a terminal row does not leak)
 *       delta = fma(g, boot, reward[n]) - value[n]
 *       carry = nt ? fma(gl, carry, delta) : delta
 *       advantage[n] = carry;  returns[n] = carry + value[n]
 * One launch of gae_kernel on `stream`, one environment per lane; the same call gives the same bits on every run.
 *   reward [K][B], value [K + 1][B] of the working dtype;  terminated, reset: [K][B] bytes (non-zero: set) at any byte offset, or NULL
 *   for never;  advantage: (out) [K][B];  returns: (out) [K][B] or NULL
 * Never allocates or synchronises. B == 0 or K == 0 returns EXCENV_OK without a launch. excenv_last_launch() reports "gae_kernel".
 * Validated before any HIP call: EXCENV_ENULL names a missing pointer (call, reward, value, advantage); EXCENV_EINVAL: dtype, B < 0,
 * K < 0, a gamma or lambda that is NaN or outside [0, 1]. */
typedef struct {
  const void* reward;         /* [K][B] */
  const void* value;          /* [K + 1][B] */
  const uint8_t* terminated;  /* [K][B] bytes or NULL (never) */
  const uint8_t* reset;       /* [K][B] bytes or NULL (never) */
  double gamma, lambda;       /* both in [0, 1] */
  void* advantage;            /* (out) [K][B] */
  void* returns;              /* (out) [K][B] or NULL */
} excenv_gae_t;
int excenv_gae(int dtype, int64_t B, int64_t K, const excenv_gae_t* call, void* stream);

/* ---- the clipped PPO objective of a diagonal Gaussian policy and its gradients on lane-major rows (additions, same
 * ABI version: a binder probes for the symbols). Everything is lane-major in the working dtype T: mean and sample [K][A][B]; logp,
 * logp_old, advantage, value and returns [K][B]; reset bytes [K][B] (non-zero: set) at any byte offset, or NULL for never; A = n_actions
 * is 1 .. EXCENV_MAX_ACTION. inv_std [A] and logp_const [1] are device arrays in T which the caller computes from log_std (in fp64,
 * then rounded to T):  inv_std[q] = exp(-log_std[q]),  logp_const = -sum_q log_std[q] - A/2 * log(2 pi),  so the log-probability
 * holds no transcendental. adv_norm is NULL or a device array T[2] (shift, scale); grad_scale is a device array T[2] (w, wv).
 * lo = (T)(1 - clip_eps) and hi = (T)(1 + clip_eps), both folded in double. Per sample (n, b), fused multiply-adds in the order written:
 *   z[q]  = (sample[q] - mean[q]) * inv_std[q]
 *   logp  = logp_const;  for q = 0 .. A-1:  logp = fma(-0.5 * z[q], z[q], logp)
 *   d     = logp - logp_old;   r = exp(d)                       (device exp; exp(0) == 1 exactly)
 *   a     = adv_norm ? (advantage - adv_norm[0]) * adv_norm[1] : advantage
 *   s1    = r * a;   s2 = min(max(r, lo), hi) * a;   surr = min(s1, s2);   active = !(s2 < s1)
 *   valid = !reset[n]                                           (reset == NULL: always valid)
 * excenv_gaussian_logp writes logp [K][B] (the first two lines; one launch of gaussian_logp_kernel): the collection-time pass. The
 * update runs the same instruction sequence, so an unchanged policy gives d == 0 and r == 1 exactly.
 * excenv_ppo_loss writes stats, double[EXCENV_PPO_STATS + A] on the device: sums over the valid samples, each term computed in T,
 * converted to fp64 and added in fp64:
 *   stats[0] = n = sum 1;   stats[1] = S_surr = sum surr;   stats[2] = S_vsq = sum (value - returns)^2   (0 when value is NULL)
 *   stats[3] = S_kl = sum ((r - 1) - d);   stats[4] = S_clip = sum [r < lo or r > hi]
 *   stats[5 + q] = S_gls[q] = sum (active ? -(r * a) : 0) * (z[q] * z[q] - 1)
 * Two launches on `stream`: ppo_loss_kernel, then ppo_loss_reduce_kernel; no atomics. A sample tile is EXCENV_PPO_TILE consecutive
 * environments of one row, tile number n * ceil(B / EXCENV_PPO_TILE) + b_tile; with Tn tiles and G = min(Tn, max_groups > 0 ?
 * max_groups : EXCENV_PPO_AUTO_GROUPS) workgroups of 256 lanes, workgroup g owns the tiles first(g) .. first(g + 1) - 1,
 * first(g) = g * (Tn / G) + min(g, Tn mod G). Lane l adds the samples 4 l .. 4 l + 3 of a tile in ascending order, tile after tile,
 * into its own fp64 sums; the workgroup adds its lanes by a fixed tree (within a wave lane l += lane l + 32, 16, 8, 4, 2, 1, then the
 * waves 0 .. 3 in order) and stores one partial set in the workspace; the second launch adds the G partial sets the same way, lane l
 * taking the sets l, l + 256, .. in ascending order. The order is a function of (B, K, max_groups) only, never of the device, the
 * alignment of the arrays or the optional pointers: the same call gives the same bits on every run.
 *   workspace : excenv_ppo_loss_workspace_bytes(B, K, max_groups) bytes of device memory (G * (EXCENV_PPO_STATS + EXCENV_MAX_ACTION)
 *               * 8; -1 for a bad argument), 8-byte aligned; needs no initialisation
 * excenv_ppo_loss_grad writes, with w = grad_scale[0] and wv = grad_scale[1] (one launch of ppo_loss_grad_kernel, no reduction):
 *   gl            = active ? -(r * a) * w : 0
 *   grad_mean[q]  = valid ? gl * z[q] * inv_std[q] : 0          ([K][A][B]: the grad_raw operand of excenv_policy_param_grad)
 *   grad_value    = valid ? wv * (value - returns) : 0          ([K][B])
 * grad_mean or grad_value may be NULL (not both); grad_value needs value and returns. The selects are selects, not products: an
 * invalid sample's gradients are exactly 0 and it reaches no sum, whatever its inputs hold; a NaN in a valid sample reaches the sums
 * and that sample's own gradients only.
 * All three kernels use 16-byte accesses where B % 4 == 0 and every array of T is 16-byte aligned (the flag bytes as one 4-byte word
 * where reset is 4-byte aligned), element accesses otherwise, with the same samples on the same lanes either way.
 * Never allocates or synchronises. B == 0 or K == 0 returns EXCENV_OK without a launch: nothing is written, stats included.
 * excenv_last_launch() reports "gaussian_logp_kernel", "ppo_loss_kernel", "ppo_loss_grad_kernel". Validated before any HIP call:
 * EXCENV_ENULL names a missing pointer; EXCENV_EINVAL: value and returns not both or neither, n_actions outside 1 .. 2, dtype, B < 0,
 * K < 0, a clip_eps that is NaN or outside (0, 1), max_groups < 0, a workspace that is too small or misaligned (with the byte count),
 * K * n_actions >= 2^31 rows. */
#define EXCENV_PPO_STATS 5             /* n, S_surr, S_vsq, S_kl, S_clip; S_gls[A] follows */
#define EXCENV_PPO_TILE 1024           /* samples of one tile: consecutive environments of one row, four to a lane */
#define EXCENV_PPO_AUTO_GROUPS 2048    /* workgroups of max_groups == 0, at most */
typedef struct {
  const void* mean;        /* [K][A][B] */
  const void* sample;      /* [K][A][B]: the pre-clamp action */
  const void* inv_std;     /* device T[A] */
  const void* logp_const;  /* device T[1] */
  int32_t n_actions;       /* A: 1 .. EXCENV_MAX_ACTION */
  void* logp;              /* (out) [K][B] */
} excenv_gaussian_logp_t;
int excenv_gaussian_logp(int dtype, int64_t B, int64_t K, const excenv_gaussian_logp_t* call, void* stream);
typedef struct {
  const void* mean;        /* [K][A][B] */
  const void* sample;      /* [K][A][B] */
  const void* inv_std;     /* device T[A] */
  const void* logp_const;  /* device T[1] */
  const void* logp_old;    /* [K][B] */
  const void* advantage;   /* [K][B] */
  const void* value;       /* [K][B] or NULL (with returns) */
  const void* returns;     /* [K][B] or NULL (with value) */
  const uint8_t* reset;    /* [K][B] bytes or NULL (never) */
  const void* adv_norm;    /* device T[2] (shift, scale) or NULL */
  int32_t n_actions;       /* A: 1 .. EXCENV_MAX_ACTION */
  int32_t max_groups;      /* excenv_ppo_loss: 0 auto; > 0: at most this many workgroups */
  double clip_eps;         /* in (0, 1) */
  double* stats;           /* excenv_ppo_loss: (out) device double[EXCENV_PPO_STATS + A] */
  void* workspace;         /* excenv_ppo_loss: excenv_ppo_loss_workspace_bytes bytes of device memory, 8-byte aligned */
  int64_t workspace_bytes;
  const void* grad_scale;  /* excenv_ppo_loss_grad: device T[2] (w, wv) */
  void* grad_mean;         /* excenv_ppo_loss_grad: (out) [K][A][B] or NULL */
  void* grad_value;        /* excenv_ppo_loss_grad: (out) [K][B] or NULL */
} excenv_ppo_loss_t;
int64_t excenv_ppo_loss_workspace_bytes(int64_t B, int64_t K, int32_t max_groups);
int excenv_ppo_loss(int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t* call, void* stream);
int excenv_ppo_loss_grad(int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t* call, void* stream);

/* ---- rollout statistics on lane-major rows (additions, same ABI version: a binder probes for the symbols): the
 * masked column moments a normalisation needs, and the returns and lengths of the episodes a rollout finished. T is the working
 * dtype; every sum is fp64. No atomics; the same call gives the same bits on every run. Neither entry allocates or synchronises.
 *
 * excenv_row_moments: masked column moments of lane-major rows.
 *   x      : [N][C][B] in T, C = n_columns = 1 .. EXCENV_MOMENTS_MAX_COLUMNS
 *   mask   : [N][B] bytes at any byte offset, non-zero = sample excluded; or NULL (none excluded)
 *   shift  : device double[C] or NULL (zeros)
 *   stats  : (out) device double[1 + 2 C]
 *   per valid sample (n, b) and column c, all in fp64:
 *       d = (double)x[n][c][b] - shift[c];   S1[c] += d;   S2[c] += d * d      (the product rounded, then added)
 *   stats[0] = number of valid samples;  stats[1 + c] = S1[c];  stats[1 + C + c] = S2[c]
 * The exclusion is a select: an excluded sample reaches no sum whatever it holds, and a NaN in a valid sample reaches the sums of its
 * own column only. Two launches on `stream`: row_moments_kernel, then rollout_stats_reduce_kernel. The tiles and workgroups are
 * excenv_ppo_loss's with K = N: a tile is EXCENV_PPO_TILE consecutive environments of one row, tile number n * ceil(B /
 * EXCENV_PPO_TILE) + b_tile; with Tn tiles and G = min(Tn, max_groups > 0 ? max_groups : EXCENV_PPO_AUTO_GROUPS) workgroups of 256
 * lanes, workgroup g owns the tiles first(g) .. first(g + 1) - 1, first(g) = g * (Tn / G) + min(g, Tn mod G). Lane l adds the samples
 * 4 l .. 4 l + 3 of a tile in ascending order, tile after tile, into its own fp64 sums; the workgroup adds its lanes by a fixed tree
 * (within a wave lane l += lane l + 32, 16, 8, 4, 2, 1, then the waves 0 .. 3 in order) and stores one partial set in the workspace;
 * the second launch adds the G sets the same way, lane l taking the sets l, l + 256, .. in ascending order. The order is a function of
 * (B, N, C, max_groups) only. 16-byte accesses where B % 4 == 0 and x is 16-byte aligned (the mask as one 4-byte word where B % 4 == 0
 * and it is 4-byte aligned), element accesses otherwise, with the same samples on the same lanes either way.
 *   workspace : excenv_row_moments_workspace_bytes(B, N, C, max_groups) bytes of device memory (G * (1 + 2 C) * 8; -1 for a bad
 *               argument), 8-byte aligned; needs no initialisation
 * B == 0 or N == 0 returns EXCENV_OK without a launch: nothing is written, stats included. excenv_last_launch() reports
 * "row_moments_kernel". Validated before any HIP call: EXCENV_ENULL names a missing pointer (call, x, stats, workspace);
 * EXCENV_EINVAL: dtype, B < 0, N < 0, n_columns out of range, max_groups < 0, a workspace that is too small or misaligned (with the
 * byte count), N * n_columns >= 2^31 rows. */
#define EXCENV_MOMENTS_MAX_COLUMNS 16
typedef struct {
  const void* x;           /* [N][C][B] */
  const uint8_t* mask;     /* [N][B] bytes or NULL (none excluded) */
  const double* shift;     /* device double[C] or NULL (zeros) */
  int32_t n_columns;       /* C: 1 .. EXCENV_MOMENTS_MAX_COLUMNS */
  int32_t max_groups;      /* 0 auto; > 0: at most this many workgroups */
  double* stats;           /* (out) device double[1 + 2 C] */
  void* workspace;         /* excenv_row_moments_workspace_bytes bytes of device memory, 8-byte aligned */
  int64_t workspace_bytes;
} excenv_row_moments_t;
int64_t excenv_row_moments_workspace_bytes(int64_t B, int64_t N, int32_t n_columns, int32_t max_groups);
int excenv_row_moments(int dtype, int64_t B, int64_t N, const excenv_row_moments_t* call, void* stream);

/* excenv_episode_stats: returns and lengths of the episodes a rollout finished, in the convention of excenv_sim_policy_episodes:
 * reward[n] belongs to row n + 1; reset[n] != 0 says the episode ended at row n and transition n is no step, so its reward is dropped.
 * Per environment b:
 *   ret = return_in[b] (double; 0 where NULL);   len = steps_in[b] (int32; 0 where NULL)
 *   for n = 0 .. K-1:
 *       if reset[n]:
 *           if len > 0:  emit (ret, len);  completed[n][b] = ret   else: completed[n][b] = 0
 *           ret = 0;  len = 0
 *       else:
 *           ret = ret + (double)reward[n];  len += 1;  completed[n][b] = 0
 *   return_out[b] = ret;  steps_out[b] = len
 *   emit(R, L):  cnt += 1;  SR += R;  SRR += R * R;  SL += L;  mn = R < mn ? R : mn;  mx = R > mx ? R : mx
 *   stats = double[EXCENV_EPISODE_STATS]: cnt, SR, SRR, SL, mn (+inf when cnt == 0), mx (-inf)
 * An episode with no transition is not an episode (a reset state that is itself terminal; every step a reset). The comparisons are as
 * written, so a NaN return is never selected as min or max. A NaN in a dropped reward changes no bit anywhere; a NaN in a counted
 * reward reaches that environment's ret, its completed entry, SR and SRR, and nothing else. With the episode_steps_in a rollout was
 * given, steps_out is its episode_steps_out.
 *   reward [K][B] in T;  reset [K][B] bytes at any byte offset, required;  return_in double[B], steps_in int32[B]: or NULL
 *   completed (out) double [K][B], return_out (out) double[B], steps_out (out) int32[B]: each may be NULL;  stats (out) double[6]
 * Two launches on `stream`: episode_stats_kernel, one environment per lane in workgroups of 256 lanes with the loads of
 * several rows in flight ahead of the scan, each environment adding its episodes in row order into its own six values; the workgroup
 * combines its lanes by the fixed tree above (min and max by the same tree with the comparisons as written) into one partial set of
 * the workspace; rollout_stats_reduce_kernel combines the ceil(B / 256) sets the same way. The order is a function of B only.
 *   workspace : excenv_episode_stats_workspace_bytes(B) bytes of device memory (ceil(B / 256) * EXCENV_EPISODE_STATS * 8; -1 for a bad
 *               argument), 8-byte aligned; needs no initialisation
 * B == 0 or K == 0 returns EXCENV_OK without a launch: nothing is written. excenv_last_launch() reports "episode_stats_kernel".
 * Validated before any HIP call: EXCENV_ENULL names a missing pointer (call, reward, reset, stats, workspace); EXCENV_EINVAL: dtype,
 * B < 0, K < 0, a workspace that is too small or misaligned (with the byte count); EXCENV_EUNSUPPORTED: a batch of 2^39 or more. */
#define EXCENV_EPISODE_STATS 6         /* cnt, SR, SRR, SL, mn, mx */
typedef struct {
  const void* reward;       /* [K][B] */
  const uint8_t* reset;     /* [K][B] bytes */
  const double* return_in;  /* [B] or NULL (zeros) */
  const int32_t* steps_in;  /* [B] or NULL (zeros) */
  double* completed;        /* (out) [K][B] or NULL */
  double* return_out;       /* (out) [B] or NULL */
  int32_t* steps_out;       /* (out) [B] or NULL */
  double* stats;            /* (out) device double[EXCENV_EPISODE_STATS] */
  void* workspace;          /* excenv_episode_stats_workspace_bytes bytes of device memory, 8-byte aligned */
  int64_t workspace_bytes;
} excenv_episode_stats_t;
int64_t excenv_episode_stats_workspace_bytes(int64_t B);
int excenv_episode_stats(int dtype, int64_t B, int64_t K, const excenv_episode_stats_t* call, void* stream);

/* ---- batched LQR synthesis: the Riccati recursion on stored linearisations (an addition, same ABI version: a binder
 * probes for the symbol). The backward pass of finite-horizon LQR, which is also the backward pass of iLQR, per environment over N rows
 * of discrete-time Jacobians. Model-free: S = n_state and A = n_action are the caller's, (S, A) one of (1, 1), (2, 1), (4, 1), (7, 2);
 * any other shape is EXCENV_EUNSUPPORTED. Everything is lane-major in the working dtype T:
 *   jac    : [N][S][S + A][B] with jac_row_stride elements between rows; element (n, i, c, b) is F_n[i][c] for c < S and G_n[i][c - S]
 *            otherwise (x+ = F_n x + G_n u): the allocation excenv_step_jacobian writes for EXCENV_JAC_STATE rows, read in place.
 *            jac_row_stride == 0: one [S][S + A][B] block read for every row (the time-invariant problem iterated N times)
 *   Q, Qf  : device T[S][S] shared by every environment and row; Qf == NULL means Q.  R : device T[A][A], likewise. All three are taken
 *            as symmetric: only the elements [i][j] with i <= j are read
 *   q      : [N + 1][S][B] or NULL (zeros);  r : [N][A][B] or NULL (zeros): the linear cost terms
 *   reg    : >= 0, added as (T)reg to the diagonal of Quu for the solve only
 *   store_all : 1: gain and ff have N rows; 0: one row, that of n = 0 (the stationary use)
 *   gain   : (out) [N or 1][A][S][B], required;  ff : (out) [N or 1][A][B];  P0 : (out) [S][S][B];  p0 : (out) [S][B];
 *            dV : (out) [2][B];  n_bad : (out) int32 [B]; each but gain may be NULL
 * Per environment b, in T, with -ffp-contract=off: every sum runs in ascending index order, a fused multiply-add appears exactly where
 * `fma` is written, `*` `+` `-` `/` are the plain rounded operations, and "s = c; k: s = fma(x_k, y_k, s)" means the chain over
 * k = 0 .. S-1 (a: over a = 0 .. A-1) in ascending order starting from c; "s = x_0 * y_0; k >= 1: ..." starts from the rounded product.
 *   P[i][j] = Qf[min(i,j)][max(i,j)];  p[i] = q[N][i];  dV0 = dV1 = 0;  bad = 0
 *   for n = N-1 down to 0, F = F_n, G = G_n:
 *       W[i][j]   = P[i][0] * F[0][j];   k >= 1: W[i][j]  = fma(P[i][k], F[k][j], W[i][j])             (W = P F)
 *       Wb[i][a]  = P[i][0] * G[0][a];   k >= 1: Wb[i][a] = fma(P[i][k], G[k][a], Wb[i][a])            (Wb = P G)
 *       Qxx[i][j] = Q[i][j];             k: Qxx[i][j] = fma(F[k][i], W[k][j], Qxx[i][j])               (i <= j only)
 *       Qux[a][j] = G[0][a] * W[0][j];   k >= 1: Qux[a][j] = fma(G[k][a], W[k][j], Qux[a][j])
 *       Quu[a][c] = R[a][c];             k: Quu[a][c] = fma(G[k][a], Wb[k][c], Quu[a][c])              (a <= c only; Quu[1][0] = Quu[0][1])
 *       Qx[i]     = q[n][i];             k: Qx[i] = fma(F[k][i], p[k], Qx[i])
 *       Qu[a]     = r[n][a];             k: Qu[a] = fma(G[k][a], p[k], Qu[a])
 *       solve (Quu + reg I) [K | k] = -[Qux | Qu] by LDL^T without square roots; for each right-hand column g (g = -Qux[.][j] -> K[.][j],
 *       g = -Qu -> k):
 *         A = 1:  d0 = Quu[0][0] + reg;  ok = d0 > 0;  x0 = g0 / d0
 *         A = 2:  d0 = Quu[0][0] + reg;  l = Quu[0][1] / d0;  d1 = fma(-l, Quu[0][1], Quu[1][1] + reg);  ok = d0 > 0 && d1 > 0
 *                 y1 = fma(-l, g0, g1);  x1 = y1 / d1;  x0 = fma(-l, x1, g0 / d0)
 *       if !ok:  K = 0, k = 0, bad += 1          (a select, a NaN compares false: the step is then open loop)
 *       QK[a][j]  = Quu[a][0] * K[0][j];   A = 2: QK[a][j] = fma(Quu[a][1], K[1][j], QK[a][j])         (the unregularised Quu)
 *       Qk[a]     = Quu[a][0] * k[0];      A = 2: Qk[a]    = fma(Quu[a][1], k[1], Qk[a])
 *       P[i][j]   = Qxx[i][j];  a: P[i][j] = fma(K[a][i], QK[a][j], P[i][j]);  a: P[i][j] = fma(K[a][i], Qux[a][j], P[i][j]);
 *                   a: P[i][j] = fma(Qux[a][i], K[a][j], P[i][j])                                      (i <= j; P[j][i] = P[i][j])
 *       p[i]      = Qx[i];  a: p[i] = fma(K[a][i], Qk[a], p[i]);  a: p[i] = fma(K[a][i], Qu[a], p[i]);  a: p[i] = fma(Qux[a][i], k[a], p[i])
 *       a: dV0 = fma(k[a], Qu[a], dV0);   h = k[0] * Qk[0];  A = 2: h = fma(k[1], Qk[1], h);   dV1 = dV1 + 0.5 * h
 *       gain[n] = K;  ff[n] = k           (store_all == 0: row 0 of gain and ff, written at n = 0 only)
 *   P0 = P;  p0 = p;  dV = (dV0, dV1);  n_bad = bad
 * So P = Qxx + K^T Quu K + K^T Qux + Qux^T K and p = Qx + K^T Quu k + K^T Qu + Qux^T k, dV0 = sum_n k . Qu and dV1 = 1/2 sum_n k . Quu k:
 * the two numbers of an iLQR line search. An environment's values reach no other environment.
 * One launch of riccati_kernel on `stream`: one environment per lane in workgroups of 256 lanes, every access one element per lane
 * and coalesced along the batch; no atomics, no reduction across lanes: the same call gives the same bits on every run. Never
 * allocates or synchronises. B == 0 returns EXCENV_OK without a launch; N == 0 writes P0 = Qf, p0 = q[0], dV = 0, n_bad = 0 and no row of
 * gain or ff. excenv_last_launch() reports "riccati_kernel". Validated before any HIP call: EXCENV_ENULL names a missing pointer (call,
 * jac, Q, R, gain); EXCENV_EINVAL: dtype, B < 0, N < 0, a reg that is negative or NaN, store_all outside 0 / 1, a jac_row_stride that
 * is neither 0 nor >= S (S + A) B; EXCENV_EUNSUPPORTED: a shape without an instantiation, a batch of 2^39 or more.
 * excenv_lqr_backward_bytes: the algorithmic bytes per environment and row of such a call (the Jacobian row unless time_invariant, the
 * q and r rows where given, the gain and ff rows where store_all); -1 for a bad argument. */
typedef struct {
  int32_t n_state, n_action;  /* S, A */
  const void* jac;            /* [N][S][S + A][B], jac_row_stride elements between rows */
  int64_t jac_row_stride;     /* 0 (one block for every row) or >= S (S + A) B */
  const void* Q;              /* device T[S][S] */
  const void* Qf;             /* device T[S][S] or NULL (Q) */
  const void* R;              /* device T[A][A] */
  const void* q;              /* [N + 1][S][B] or NULL (zeros) */
  const void* r;              /* [N][A][B] or NULL (zeros) */
  double reg;                 /* >= 0 */
  int32_t store_all;          /* 1: every row of gain and ff; 0: row 0 only */
  void* gain;                 /* (out) [N or 1][A][S][B] */
  void* ff;                   /* (out) [N or 1][A][B] or NULL */
  void* P0;                   /* (out) [S][S][B] or NULL */
  void* p0;                   /* (out) [S][B] or NULL */
  void* dV;                   /* (out) [2][B] or NULL */
  int32_t* n_bad;             /* (out) [B] or NULL */
} excenv_lqr_t;
int excenv_lqr_backward(int dtype, int64_t B, int64_t N, const excenv_lqr_t* call, void* stream);
int64_t excenv_lqr_backward_bytes(int dtype, int32_t n_state, int32_t n_action, int time_invariant, int has_q, int has_r, int store_all,
                                  int has_ff);

/* ---- replaces CoreEnvironment.vmap_generate_state_from_observation (core_env.py:689-705; per env e.g.
 * pendulum_env.py:331-364, pmsm_env.py:921-970): obs [B][O + n_control] row-major -> denormalised physical state leaves
 * state_out[S][B] and, for each controlled field control_idx[j], its denormalised reference leaf reference_out[j][B]
 * (the other reference leaves are NaN by definition and are not written here). */
int excenv_state_from_observation(int env, int dtype, int64_t B, const excenv_props_t* props, int32_t n_control,
                                  const int32_t* control_idx, const void* obs, void* const* state_out,
                                  void* const* reference_out, void* stream);

/* ---- replaces GymWrapper.update_ref / generate_new_ref (gym_wrapper.py:170-192), one thread per environment: where
 * hold[i] == 0 draw a random initial state from the environment's key (init_state(rng), e.g. pendulum_env.py:270-276, PMSM
 * pmsm_env.py:402-456 incl. jax.random.ball), copy its controlled fields into reference[j][i], split the key for the new hold
 * time (jax.random.randint(sub, (1,), hold_steps_min, hold_steps_max) in the default int type: the int32 form for EXCENV_F32, the
 * int64 form JAX draws under jax_enable_x64 for EXCENV_F64 — float64 arrays exist in the reference only with x64 on) and keep the
 * other half as the new key; then hold[i] -= 1. All arrays are updated in place. keys: [B][2] uint32 key words stored in int64
 * (jax.random key data). The samplers restate JAX's published algorithms (threefry2x32 split / bits / uniform / randint / normal /
 * gamma / ball); the CPU oracle's restatement of the same functions is pinned on the Random123 known-answer vectors and on the
 * jax.random.split / normal values printed in JAX's documentation (tests/test_oracle_rng.py), and these kernels are compared
 * with that oracle (tests/test_gpu_rng_oracle.py). Unpinned: the x64 form of randint (no published value; checked against a
 * big-integer restatement). */
int excenv_update_ref(int env, int dtype, int64_t B, const excenv_props_t* props, int32_t n_control,
                      const int32_t* control_idx, void* const* reference, int64_t* keys, int64_t* hold,
                      int32_t hold_steps_min, int32_t hold_steps_max, void* stream);

/* ---- replaces CoreEnvironment.generate_observation vmapped over the batch (e.g. pendulum_env.py:311-329, PMSM
 * pmsm_env.py:898-919; used by vmap_reset, core_env.py:665-687): obs [B][O + n_control] row-major = the normalised physical
 * state in the environment's observation order followed by the normalised reference of each controlled field
 * (control->reference[j], NaN allowed). The same device function the step / trajectory kernels fuse. */
int excenv_observe(int env, int dtype, int64_t B, const excenv_props_t* props, const excenv_control_t* control,
                   const void* const* state, void* obs, void* stream);

/* Out-of-place form of excenv_update_ref (the functional contract of GymWrapper.update_ref, gym_wrapper.py:170-175: the
 * incoming state is not modified): reads reference_in / keys_in / hold_in, writes every environment's values — redrawn or
 * carried over — to reference_out / keys_out / hold_out. Outputs must not alias the inputs. */
int excenv_update_ref_to(int env, int dtype, int64_t B, const excenv_props_t* props, int32_t n_control,
                         const int32_t* control_idx, const void* const* reference_in, const int64_t* keys_in,
                         const int64_t* hold_in, void* const* reference_out, int64_t* keys_out, int64_t* hold_out,
                         int32_t hold_steps_min, int32_t hold_steps_max, void* stream);

/* ---- replaces CoreEnvironment.vmap_init_state(rng) (core_env.py:649-662) with one key per environment: the random branch
 * of each environment's init_state (e.g. pendulum_env.py:270-276, PMSM pmsm_env.py:402-456) — state_out[S][B] physical state
 * leaves, key_leaf [B][2] the keys that become State.PRNGKey. Same samplers as excenv_update_ref. */
int excenv_random_state(int env, int dtype, int64_t B, const excenv_props_t* props, const int64_t* keys,
                        void* const* state_out, int64_t* key_leaf, void* stream);

/* ---- the path's one collective (no reference counterpart: the reference is single-device): all ranks integrate
 * their own contiguous slice of the batch with no communication, and a consumer that needs the global batch on every rank
 * reassembles it with ONE all-gather — typically the last observation row of a chunk (obs_traj + N * (O + n_control) * B elements
 * in the lane-major layout: count_per_rank = (O + n_control) * B_local). A thin wrapper over RCCL's ncclAllGather for binders
 * that do not go through torch.distributed (the Python mirror does): `nccl_comm` is the caller's ncclComm_t, `recv` holds
 * world_size * count_per_rank elements in rank order, enqueued on `stream`. librccl.so is loaded on first use; without it the
 * call returns EXCENV_EUNSUPPORTED. Shards must be equal-sized (pad the last rank's slice otherwise). */
int excenv_allgather(void* nccl_comm, int dtype, const void* send, void* recv, int64_t count_per_rank, void* stream);

/* ---- calibration, no reference counterpart: the memory access shape of excenv_sim_ahead (lane-major buffers) without any
 * arithmetic. `rows` times, every workgroup reads one 4 KiB piece of each of n_read streams and writes one 4 KiB piece of each
 * of n_write streams (16 bytes per lane, 256 lanes); stream s covers bytes [0, row_bytes) of its row and advances by its own
 * row stride: for a trajectory call the read streams are the A action components (base actions + c*B*w, row stride A*B*w), the
 * write streams the O observation components (base obs + c*B*w, row stride O*B*w) and the S state leaves (row stride B*w), with
 * row_bytes = B*w and rows = K*substeps. What is written is meaningless: use it on buffers whose contents are dead. It tells,
 * in the same process and over the very buffers of a trajectory call, how fast HBM takes that traffic where the driver placed
 * those buffers (bench.py: roofline.same_run_pattern_gbs; the Python mirror uses it to reject slow placements of large
 * trajectory buffers before the first trajectory is written). n_read <= 4, n_write <= 32; bases and strides
 * 16-byte aligned; nontemporal != 0 selects the streaming stores the trajectory kernels use. */
int excenv_stream_pattern(int32_t n_read, const void* const* read_base, const int64_t* read_row_stride_bytes,
                          int32_t n_write, void* const* write_base, const int64_t* write_row_stride_bytes,
                          int64_t row_bytes, int64_t rows, int32_t nontemporal, void* stream);

/* ---- device-math probes (tests only): out[i] = f(in[i]) for the in-kernel routines. 0 / 1 / 2 in either dtype (the forward
 * kernels' sin, cos and wrap_angle); 3 / 4 are sin and cos through the reverse-mode kernels' fp64 routine (devmath.hpp
 * sincos_lean): EXCENV_F64 only, EXCENV_EINVAL otherwise. -- */
int excenv_probe_math(int which /*0 sin,1 cos,2 wrap_angle,3 lean sin,4 lean cos*/, int dtype, int64_t n,
                      const void* in, void* out, void* stream);

/* out_fast[i] = the kernels' division by a loop-invariant denominator (devmath.hpp InvDiv) of num[i] by den[i];
 * out_ref[i] = num[i] / den[i] as the compiler expands it. Tests assert equal bits. */
int excenv_probe_div(int dtype, int64_t n, const void* num, const void* den, void* out_fast, void* out_ref, void* stream);

#define EXCENV_OK 0
#define EXCENV_EINVAL (-1)  /* bad enum / size / combination */
#define EXCENV_ENULL (-2)   /* required pointer is NULL */
#define EXCENV_EHIP (-3)    /* HIP runtime error at launch */
#define EXCENV_EUNSUPPORTED (-4)

#ifdef __cplusplus
}
#endif
#endif /* EXCENV_H */
