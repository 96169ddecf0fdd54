// Which form of the trajectory kernel one excenv_sim_ahead[_ws] call runs: decided here, once, from plain facts about the call
// (sim_plan), and nowhere else. Host-only and free of HIP: the host C++ compiler builds it alone (tests/test_sim_plan.py).
// The model constants the choice reads live here as constexpr functions of plain values; the kernel headers use the same ones.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/excenv.h"

namespace excenv {

constexpr int BLOCK = 256;
constexpr int EM_LANES = 64;  // one wave per workgroup (the env-major kernels)
static_assert(EXCENV_TILE % BLOCK == 0, "a workgroup must not straddle tiles of the tiled layout");
// steps per flush window of the LDS-ring kernel for 4-byte elements (8-byte: half): the LDS ring of TK saved states per environment
// decides how many waves fit a CU: TK = 8 -> 26.5 KB per wave (PMSM), six waves per CU; TK = 16 -> 41 KB, three
constexpr int EM_TK = 8;
constexpr int EMR_MAX_RING_REGS = 128;  // register budget of the register ring's 128-byte windows (4-byte elements; emr_rows)

// Environments per lane by batch size (small batches: one, the per-step dependent chain of a wave as short as possible). Two per
// lane from one wave per SIMD on the chip (1024 SIMDs x 64 lanes), FOUR only from two waves per SIMD: at B = 2^18 four per lane leave one 256-thread workgroup per CU — round 4, same-buffers A/B and fresh processes:
// PMSM Euler 0.411 -> 0.325 ms with two per lane, pendulum 1.259 -> 0.963, cart-pole 0.228 -> 0.153; from 2^19 on four win.
constexpr int auto_envs_per_lane(int64_t B, int vmax) {
  while (vmax > 1 && (B / vmax) < (int64_t)1024 * 64 * (vmax >= 4 ? 2 : 1)) vmax >>= 1;
  return vmax;
}
// The forms that exist only at the widest lane width (row-major actions read by the kernel, lean gym outputs) keep the earlier bound:
// they beat what the call would fall back to (a transposition pass, the one-environment general kernel) from one wave per SIMD on.
constexpr bool widest_form_pays(int64_t B, int vmax) { return (B / vmax) >= (int64_t)1024 * 64; }

constexpr int64_t ROW_SYNC_MIN_BATCH = (int64_t)1 << 17;  // one environment per lane: rows stored together from this batch on
// Threads per workgroup of the plain lean trajectory kernel (kernels.hpp, NT): 1024 with one barrier per row for the Euler kernels of
// the small models, BLOCK everywhere else — measured per workload (profiles/r04_pattern_sweep.md): pendulum Euler fp32 -10.6 %, fp64
// -8 %, MSD Euler fp32 -7 %, fp64 -6 %, tank Euler fp32 -6 % (fp64 +3 %: not taken); RK4 / Tsit5 of the same models +3 ... +9 %,
// cart-pole / acrobot Euler within 3 % either way, PMSM (256 registers) not possible.
constexpr int WIDE_THREADS = 1024;
constexpr int64_t WIDE_MIN_WORKGROUPS = 256;  // at least one wide workgroup per CU of the MI355X, else the narrow form fills the chip better
constexpr bool sim_wide_ok(int env, int elem, int solver, bool lut) {
  return solver == EXCENV_EULER && !lut &&
         (env == EXCENV_PENDULUM || env == EXCENV_MASS_SPRING_DAMPER || (env == EXCENV_FLUID_TANK && elem == 4));
}
// with the gym outputs' code the fp64 pendulum instantiations need 146 ... 150 registers: they would spill under the 1024-thread bound
// (fp32: 118 ... 123 since round 5 — wide like its plain launch: 2.43 -> 2.2 ms for the gym trajectories of B = 2^22, K = 100)
constexpr bool sim_wide_gym_ok(int env, int elem, int solver, bool lut) {
  return sim_wide_ok(env, elem, solver, lut) && (env != EXCENV_PENDULUM || elem == 4);
}
// Row-major actions read by the lean kernel (kernels.hpp, AEM): a lane's V environments' A values must fill whole 16-byte pieces
constexpr bool aem_fits(int A, int elem) { return (16 / elem) % A == 0; }
// The LDS-ring env-major kernel (kernels_em.hpp): steps per flush window and LDS elements per wave — the per-lane action line
// (128 bytes + one 16-byte pad), the ring of saved states, one round of observation rows
constexpr int em_tk(int elem) { return elem == 4 ? EM_TK : EM_TK / 2; }
constexpr size_t em_lds_elems(int elem, int S, int O) { return (size_t)EM_LANES * (128 / elem + 16 / elem + S * (em_tk(elem) + 1) + O); }
// The register-ring env-major kernel (kernels_emr.hpp). Leaves that need no window: one that never changes along a trajectory —
// PMSM's omega_el (pmsm_env.py:509-523: the ODE has no equation for it; sim_ahead keeps it constant, :785-791) — and one that is a
// function of other saved leaves: PMSM's torque in the reference-structured trajectory, where every saved row is post-processed
// (pmsm_env.py:573-578, 680-688: torque from the saved currents; the same device function M::torque here). On the step-semantics path
// row 0 carries the caller's torque as it came in, so there it stays in the ring. -1: none.
constexpr bool emr_supported(bool lut) { return !lut; }  // the look-up model keeps the LDS-ring kernel
constexpr int emr_const_leaf(bool pmsm) { return pmsm ? 6 : -1; }
constexpr int emr_derived_leaf(bool pmsm, bool ahead) { return (pmsm && ahead) ? 5 : -1; }
constexpr int emr_ring_leaves(int S, bool pmsm, bool ahead) {
  return S - (emr_const_leaf(pmsm) >= 0 ? 1 : 0) - (emr_derived_leaf(pmsm, ahead) >= 0 ? 1 : 0);
}
// Steps per window. Two waves must share a SIMD (one wave alone leaves the VALU half idle: 9.9 ms for the headline launch with
// 128-byte windows at one wave per SIMD, 7.7 ms with 64-byte windows at two), so a lane has 256 registers and the windows of
// all ring leaves must fit next to the integration's own: 128-byte runs (whole lines, 32 registers per leaf) while the ring
// stays within EMR_MAX_RING_REGS, else 64-byte runs (half lines, written 4 lanes x 16 bytes). PMSM in fp64 (5 ... 6 leaves
// x 8 doubles next to a double-precision integration) fits since the torque leaf left the ring and the action line is loaded at
// the crossing: two registers are spilled, reloaded only on the IEEE-division fallback path of the flush.
constexpr int emr_rows(int S, bool pmsm, bool ahead, int elem) {  // a double-precision integration needs twice the registers itself
  return (emr_ring_leaves(S, pmsm, ahead) * 32 <= EMR_MAX_RING_REGS / (elem / 4) ? 128 : 64) / elem;
}
// Environments between consecutive lanes of a register-ring wave: the period in e of the window phase (e * (K + 1)) % W
constexpr int64_t emr_period(int64_t K, int64_t W) {
  int64_t g = W, y = (K + 1) % W;
  while (y) { const int64_t t = g % y; g = y; y = t; }
  return W / g;
}
constexpr int64_t align_up(int64_t x) { return (x + 255) & ~(int64_t)255; }
// Workspace for the transposition path: the actions and / or the trajectories of env-major buffers, 256-byte aligned each
constexpr int64_t sim_workspace_bytes(int S, int A, int O, int elem, int64_t B, int64_t K, int32_t substeps, int32_t n_control,
                                      int action_layout, int traj_layout, bool with_state_traj) {
  const int64_t rows = K * substeps + 1;
  return (action_layout == EXCENV_LAYOUT_ENV_MAJOR ? align_up(elem * K * A * B) : 0) +
         (traj_layout == EXCENV_LAYOUT_ENV_MAJOR ? align_up(elem * rows * (O + n_control) * B) +
                                                       (with_state_traj ? S * align_up(elem * rows * B) : 0) : 0);
}
// Largest power of two up to 128 that divides the address (NULL: 128)
inline int align_of(const void* p) { const uintptr_t a = reinterpret_cast<uintptr_t>(p) | 128u; return (int)(a & (~a + 1)); }
// Everything the choice depends on. Alignments are align_of() of the pointers (the least over a group).
struct SimFacts {
  int env, S, A, O, elem, solver, semantics;
  int64_t B, K;
  int32_t substeps; int action_layout, traj_layout;
  bool per_env_props, lut;  // some property given per environment; saturated PMSM (look-up tables attached)
  int n_control; bool refs_given, gym, state_traj;  // every control->reference[j] non-NULL; gym / state trajectories requested
  int al_actions, al_obs, al_state_io, al_straj;  // al_state_io: state_in and last_state; al_straj: 128 without state_traj
  int al_reward, al_terminated, al_truncated, al_refs;
  int envs_per_lane, env_major_mode, flags;  // excenv_launch_opts_t
  bool workspace; int al_workspace; int64_t workspace_bytes;  // a workspace pointer was given; its alignment and size
};
// sim_ahead_kernel: GENERAL (one environment per lane: any layout, per-env properties, control columns, gym outputs), LEAN (V per
// lane, 256 or 1024 threads), LEAN_GYM (widest V with the gym outputs' code), AEM (widest V reading row-major actions itself);
// env-major buffers: EM (LDS-ring kernel, kernels_em.hpp; EM_GENERAL with per-env properties or control columns), EMR (register ring)
enum SimForm { SIM_GENERAL, SIM_LEAN, SIM_LEAN_GYM, SIM_AEM, SIM_EM, SIM_EM_GENERAL, SIM_EMR };
struct SimPlan {
  SimForm form;
  bool via_workspace;  // transpose the env-major buffers through the workspace, run the rest of the plan on the lane-major copies
  int V, threads;      // environments per lane, threads per workgroup
  int row_sync, row_lds;  // kernels.hpp row_sync: 0 off, 1 barrier per row, 2 rows leave through LDS (row_lds bytes)
  bool split_control;  // the control columns are filled by control_fill_kernel behind the trajectory kernel
  int64_t period;      // SIM_EMR: environments between the lanes of a wave
  bool acc_t = false;  // EXCENV_SEM_AHEAD_ACCUMULATED_T: the accumulated-time instantiations of GENERAL / LEAN (kernels.hpp ACC_T)
};
// Whether launch.hpp instantiates the kernel a plan names, for a model (env id, A, look-up tables attached), element size and solver.
// The launchers emit exactly these instantiations and report any other plan as an error; tests/test_sim_plan.py checks that
// sim_plan() picks only these. The accumulated-time kernel has the GENERAL / LEAN forms only (one action row per step is what the
// row-major action windows, the fused env-major kernels and the lean gym outputs assume).
constexpr bool sim_instantiated(const SimPlan& p, int semantics, int env, int A, int elem, int solver, bool lut) {
  const bool acc_t = semantics == EXCENV_SEM_AHEAD_ACCUMULATED_T;
  if ((elem != 4 && elem != 8) || solver < 0 || solver >= EXCENV_NUM_SOLVERS || semantics < EXCENV_SEM_STEP ||
      semantics > EXCENV_SEM_AHEAD_ACCUMULATED_T || p.acc_t != acc_t)
    return false;
  const int VA = 16 / elem;  // the widest lane
  switch (p.form) {
    case SIM_GENERAL: return p.V == 1 && p.threads == BLOCK;
    case SIM_LEAN:
      if (p.threads == WIDE_THREADS) return p.V == VA && sim_wide_ok(env, elem, solver, lut);
      return p.threads == BLOCK && (p.V == 1 || p.V == 2 || (p.V == 4 && elem == 4));
    case SIM_LEAN_GYM:  // widest lane only: two environments per lane in fp32, built and measured in round 4, lost (PMSM 5.80 ->
                        // 7.26 ms, cart-pole 3.55 -> 4.34, acrobot 3.55 -> 4.11)
      return !acc_t && !lut && p.V == VA && (p.threads == BLOCK || (p.threads == WIDE_THREADS && sim_wide_gym_ok(env, elem, solver, lut)));
    case SIM_AEM: return !acc_t && !lut && aem_fits(A, elem) && p.V == VA && p.threads == BLOCK;
    case SIM_EM:
    case SIM_EM_GENERAL: return !acc_t && p.V == 1 && p.threads == EM_LANES;
    case SIM_EMR: return !acc_t && emr_supported(lut) && p.V == 1 && p.threads == EM_LANES;
  }
  return false;
}

namespace plan_detail {
constexpr int vmax(const SimFacts& f) { return 16 / f.elem; }
// EXCENV_SEM_AHEAD_ACCUMULATED_T: the action row is not step / substeps (it stays or jumps by two in some steps), so the forms that
// assume one row per step — the row-major action windows (AEM), the fused env-major kernels (EM, EM_GENERAL, EMR) — and the lean gym
// outputs have no instantiation for it; everything else is planned exactly as for EXCENV_SEM_AHEAD.
constexpr bool acc_t(const SimFacts& f) { return f.semantics == EXCENV_SEM_AHEAD_ACCUMULATED_T; }
// The lane width the widest-only forms (AEM, lean gym outputs) need is the one the call would take anyway
constexpr bool takes_widest(const SimFacts& f) {
  int want = f.envs_per_lane > 0 ? f.envs_per_lane : (widest_form_pays(f.B, vmax(f)) ? vmax(f) : 1);
  // acrobot RK4 / Tsit5: two environments per lane (below)
  if (f.envs_per_lane == 0 && f.env == EXCENV_ACROBOT && f.solver != EXCENV_EULER && want > 2) want = 2;
  return want == vmax(f);
}
// Row-major actions [B][K][A] with lane-major trajectories — what a reference-shaped vmap_sim_ahead call with the library's default
// outputs is: the widest lean instantiation reads them itself through a per-wave LDS piece ring (kernels.hpp, AEM) instead of a
// transposition pass in front of the launch. Control columns are filled behind it (control_fill_kernel reads every reference).
constexpr bool reads_row_major_actions(const SimFacts& f) {
  const int vm = vmax(f);
  if ((f.flags & EXCENV_OPT_NO_FUSED_ACTIONS) || acc_t(f) || f.lut || f.per_env_props || f.gym || !f.refs_given || f.al_obs < 16) return false;
  if (f.action_layout != EXCENV_LAYOUT_ENV_MAJOR || f.traj_layout != EXCENV_LAYOUT_LANE_MAJOR) return false;
  if (f.K < 1 || !aem_fits(f.A, f.elem) || (f.K * f.A) % vm != 0) return false;  // whole 16-byte pieces per row
  if ((f.B % (64 * vm)) != 0) return false;  // whole waves: the lanes of a wave fetch action windows for each other
  if (f.al_actions < 16) return false;
  if ((int64_t)BLOCK * vm * f.K * f.A >= ((int64_t)1 << 32)) return false;  // 32-bit element offsets inside a workgroup
  return takes_widest(f);
}
// Both layouts env-major, substeps == 1, no gym trajectories, the time tile fits LDS, the action array made of whole 16-byte pieces
constexpr bool fused_env_major(const SimFacts& f) {
  return !acc_t(f) && f.B > 0 && f.K > 0 && f.al_obs >= 16 && f.al_actions >= 16 && (f.B * f.K * f.A * f.elem) % 16 == 0 &&
         f.env_major_mode != 1 && f.action_layout == EXCENV_LAYOUT_ENV_MAJOR && f.traj_layout == EXCENV_LAYOUT_ENV_MAJOR &&
         f.substeps == 1 && !f.gym && em_lds_elems(f.elem, f.S, f.O) * f.elem <= 150 * 1024;
}
constexpr SimPlan plan_env_major(const SimFacts& f) {
  const bool general = f.per_env_props || f.n_control > 0;
  SimPlan p{general ? SIM_EM_GENERAL : SIM_EM, false, 1, EM_LANES, 0, 0, false, 0};
  // register ring (env_major_mode 0: large batches; 3: whenever its preconditions hold): whole-line stores. Needs 128-byte aligned
  // trajectory arrays, action rows of whole 16-byte pieces (fetched as 64-byte windows by LDS-direct loads) and enough
  // environments to fill waves whose lanes are P environments apart.
  if ((f.env_major_mode == 0 || f.env_major_mode == 3) && !general && emr_supported(f.lut)) {
    const int64_t P = emr_period(f.K, emr_rows(f.S, f.env == EXCENV_PMSM, f.semantics != EXCENV_SEM_STEP, f.elem));
    if (f.al_obs >= 128 && f.al_straj >= 128 && (f.env_major_mode == 3 || f.B >= 16 * EM_LANES * P) &&
        (f.K * f.A * f.elem) % 16 == 0 && f.al_actions >= 16 &&
        EM_LANES * P * (f.K + 1) * f.O * (int64_t)f.elem < ((int64_t)1 << 31))  // 32-bit lane offsets
      p = SimPlan{SIM_EMR, false, 1, EM_LANES, 0, 0, false, P};
  }
  return p;
}
constexpr SimPlan plan_lane_major(const SimFacts& f) {
  const int VMAX = vmax(f);
  const bool lm_a = f.action_layout == EXCENV_LAYOUT_LANE_MAJOR, lm_t = f.traj_layout == EXCENV_LAYOUT_LANE_MAJOR;
  const bool em_a = f.action_layout == EXCENV_LAYOUT_ENV_MAJOR, em_t = f.traj_layout == EXCENV_LAYOUT_ENV_MAJOR;
  const bool tiled = f.action_layout == EXCENV_LAYOUT_TILED || f.traj_layout == EXCENV_LAYOUT_TILED;
  const bool states16 = f.al_state_io >= 16 && f.al_straj >= 16;
  // The gym trajectories come out of the widest lean form (LGYM) when everything is lane-major, the batch runs that form anyway and
  // the arrays allow its vector accesses: truncated V * TW bytes per lane, as dwords aligned to 4 bytes when that is a multiple of 4,
  // else to 2 (kernels.hpp store_flag_bytes). Anything else takes the general kernel.
  const int TW = (f.env == EXCENV_PMSM || f.env == EXCENV_FLUID_TANK) ? 1 : f.O + f.n_control;
  const bool lean_gym = f.gym && !acc_t(f) && !f.per_env_props && !f.lut && f.n_control <= f.S && lm_a && lm_t && (f.B % VMAX) == 0 &&
                        takes_widest(f) && states16 && f.al_actions >= 16 && f.al_obs >= 16 && f.al_reward >= 16 &&
                        f.al_terminated >= VMAX && f.al_truncated >= ((VMAX * TW) % 4 == 0 ? 4 : 2) &&
                        (f.n_control == 0 || (f.refs_given && f.al_refs >= 16)) &&
                        // the four-leaf models in fp64 with an RK solver would need more than 256 registers in that form
                        !(f.elem == 8 && f.S == 4 && f.solver != EXCENV_EULER);
  const bool aem_candidate = reads_row_major_actions(f) && states16;
  // control_state columns alone (broadcast properties, no gym outputs or the lean ones, lane-major / tiled trajectories) do not need
  // the general kernel: they are constant along the trajectory and are filled by control_fill_kernel after the lean kernel has
  // written everything else (same bytes, +1 launch, 0.52 -> 0.7 of the HBM roof at B = 2^22); row-major actions the lean kernel
  // reads itself (AEM) are no reason for the general kernel either
  const bool split = !f.per_env_props && (!f.gym || lean_gym) && f.n_control > 0 && !em_t && (!em_a || aem_candidate) && f.refs_given;
  const bool general = f.per_env_props || (f.n_control > 0 && !split) || (f.gym && !lean_gym);
  const bool aem = aem_candidate && !general;
  SimPlan p{general ? SIM_GENERAL : lean_gym ? SIM_LEAN_GYM : aem ? SIM_AEM : SIM_LEAN, false, 1, BLOCK, 0, 0, split, 0};
  // one environment per lane for the general kernel (two, each with its own property set, measured no faster: DESIGN.md §4.1)
  const bool vec_ok = !general && states16 && (!em_a || aem) && !em_t && f.al_actions >= 16 && f.al_obs >= 16;
  if (vec_ok) {
    int want = f.envs_per_lane > 0 ? f.envs_per_lane : ((aem || lean_gym) ? VMAX : auto_envs_per_lane(f.B, VMAX));
    if (f.envs_per_lane == 0) {
      // acrobot RK4 / Tsit5 is VALU-bound with the largest register footprint of all instantiations: two envs per lane keep
      // a third wave per SIMD resident (measured +7 % over four)
      if (f.env == EXCENV_ACROBOT && f.solver != EXCENV_EULER && want > 2) want = 2;
      // look-up models: the interpolation code per environment is large (instruction cache) and keeps six table values per
      // environment live across the step (V = 4 needs > 256 registers): measured best at two environments per lane for Euler
      // and one for RK4 / Tsit5
      if (f.lut && want > (f.solver == EXCENV_EULER ? 2 : 1)) want = f.solver == EXCENV_EULER ? 2 : 1;
      // PMSM observations only in fp32: the arithmetic of a step is the full launch's, the bytes are 40 of 68 — VALU floor and memory
      // floor meet and what counts is how well they overlap (fewer registers, more resident waves; with full outputs four stay
      // faster: RK4 5.64 vs 6.19 ms, Tsit5 6.25 vs 6.37). Round 5, same-buffers A/B, one / two / four per lane: Euler 3.34 / 3.49 /
      // 3.46 ms — one; RK4 3.79 / 3.72 / 4.04 and Tsit5 4.32 / 4.19 / 4.73 — two.
      if (f.env == EXCENV_PMSM && !f.lut && f.elem == 4 && !f.state_traj && !aem && !lean_gym &&
          want > (f.solver == EXCENV_EULER ? 1 : 2))
        want = f.solver == EXCENV_EULER ? 1 : 2;
      // cart-pole RK4 / Tsit5 and pendulum Tsit5 in fp32: the same trade (registers for a resident wave) — same-buffers A/B with two
      // instead of four environments per lane: cart-pole RK4 4.646 -> 4.323 ms, Tsit5 7.046 -> 6.091, pendulum Tsit5 2.637 -> 2.477
      // (pendulum RK4, mass-spring-damper, tank: four stay faster or equal)
      if (f.elem == 4 && !aem && !lean_gym && want > 2 &&
          ((f.env == EXCENV_CART_POLE && f.solver != EXCENV_EULER) || (f.env == EXCENV_PENDULUM && f.solver == EXCENV_TSIT5)))
        want = 2;
    }
    if (want > VMAX) want = VMAX;
    while (want > 1 && (f.B % want) != 0) want >>= 1;
    p.V = want;
  }
  if (tiled) {  // a workgroup must not straddle tiles
    constexpr int VT = EXCENV_TILE / BLOCK;
    p.V = (VT > VMAX || !vec_ok) ? 1 : VT;
  }
  // one environment per lane at a batch that fills the chip several times over: the four waves of a workgroup store each row
  // together (kernels.hpp row_sync); with whole workgroups and aligned arrays the rows leave through LDS as 16-byte stores
  // (not with the gym outputs' code in the loop: with that much arithmetic per row lockstep costs more than the stores gain —
  // PMSM 7.06 -> 8.59 ms, pendulum 4.64 -> 5.28, acrobot 7.0 -> 8.0 measured)
  const int row_bytes = 2 * (f.O + f.n_control + (f.state_traj ? f.S : 0)) * BLOCK * f.elem;
  if (p.V == 1 && !f.gym && lm_t && f.B >= ROW_SYNC_MIN_BATCH)
    p.row_sync = (!f.lut && (f.B % BLOCK) == 0 && f.al_obs >= 16 && f.al_straj >= 16 && row_bytes <= (64 << 10)) ? 2 : 1;
  if (p.row_sync == 2) p.row_lds = row_bytes;
  if (sim_wide_ok(f.env, f.elem, f.solver, f.lut) && (!lean_gym || sim_wide_gym_ok(f.env, f.elem, f.solver, f.lut)) &&
      (p.form == SIM_LEAN || p.form == SIM_LEAN_GYM) && !tiled && p.V == VMAX && f.B / p.V >= WIDE_THREADS * WIDE_MIN_WORKGROUPS)
    p.threads = WIDE_THREADS;
  return p;
}
}  // namespace plan_detail

// One decision for the whole call: fused env-major kernel / workspace + transposes / the lane-major kernel (generic strides for
// env-major buffers it cannot take otherwise)
constexpr SimPlan sim_plan(const SimFacts& f) {
  using namespace plan_detail;
  if (fused_env_major(f)) return plan_env_major(f);
  const bool em_a = f.action_layout == EXCENV_LAYOUT_ENV_MAJOR, em_t = f.traj_layout == EXCENV_LAYOUT_ENV_MAJOR;
  const int64_t need = sim_workspace_bytes(f.S, f.A, f.O, f.elem, f.B, f.K, f.substeps, f.n_control, f.action_layout,
                                           f.traj_layout, f.state_traj);
  if (!reads_row_major_actions(f) && !f.gym && f.workspace && need > 0 && f.workspace_bytes >= need && f.B > 0 && (em_a || em_t)) {
    SimFacts w = f;  // the kernel runs on lane-major copies in the workspace (each 256-byte aligned within it)
    if (em_a) { w.action_layout = EXCENV_LAYOUT_LANE_MAJOR; w.al_actions = f.al_workspace; }
    if (em_t) { w.traj_layout = EXCENV_LAYOUT_LANE_MAJOR; w.al_obs = f.al_workspace; w.al_straj = f.state_traj ? f.al_workspace : 128; }
    w.flags = 0;
    SimPlan p = plan_lane_major(w);
    p.via_workspace = true;
    p.acc_t = acc_t(f);
    return p;
  }
  SimPlan p = plan_lane_major(f);
  p.acc_t = acc_t(f);
  return p;
}
// What excenv_last_launch() reports for a plan
constexpr const char* plan_name(const SimPlan& p) {
  const bool wide = p.threads == WIDE_THREADS;
  if (p.acc_t) {  // GENERAL / LEAN only (sim_plan)
    if (p.via_workspace) return "transposition workspace + sim_ahead_kernel (accumulated t)";
    if (p.form == SIM_GENERAL) return "sim_ahead_kernel (general, accumulated t)";
    if (p.V == 1) return "sim_ahead_kernel (V=1, accumulated t)";
    if (p.V == 2) return wide ? "sim_ahead_kernel (V=2, 1024 threads, accumulated t)" : "sim_ahead_kernel (V=2, accumulated t)";
    return wide ? "sim_ahead_kernel (V=4, 1024 threads, accumulated t)" : "sim_ahead_kernel (V=4, accumulated t)";
  }
  if (p.via_workspace) return "transposition workspace + sim_ahead_kernel";
  switch (p.form) {
    case SIM_GENERAL: return "sim_ahead_kernel (general)";
    case SIM_LEAN_GYM: return wide ? "sim_ahead_kernel (lean, gym outputs, 1024 threads)" : "sim_ahead_kernel (lean, gym outputs)";
    case SIM_AEM: return "sim_ahead_kernel (row-major actions fused)";
    case SIM_EM: return "sim_ahead_em_kernel";
    case SIM_EM_GENERAL: return "sim_ahead_em_kernel (general)";
    case SIM_EMR: return "sim_ahead_emr_kernel";
    case SIM_LEAN: break;
  }
  if (p.V == 1) return "sim_ahead_kernel (V=1)";
  if (p.V == 2) return wide ? "sim_ahead_kernel (V=2, 1024 threads)" : "sim_ahead_kernel (V=2)";
  return wide ? "sim_ahead_kernel (V=4, 1024 threads)" : "sim_ahead_kernel (V=4)";
}

}  // namespace excenv
