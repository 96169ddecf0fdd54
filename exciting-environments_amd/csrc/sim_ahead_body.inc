// The body of the trajectory kernels sim_ahead_kernel and sim_ahead_acc_t_kernel (kernels.hpp), included into both kernel
// definitions so that each instantiation is compiled as one function, as before the accumulated-time kernels existed (a shared
// __device__ function inlined into two kernels gave the existing instantiations other register allocations, some with scratch).
// In scope: the kernel's template parameters M, T, SOLVER, AHEAD, GENERAL, V, STATES, LUT_LDS, AEM, LGYM, NT, the constant
// ACC_T, the argument block `ka` and the accumulated-time clock's acc_step / acc_end (sim_clock.hpp; unused unless ACC_T).
  static_assert(!ACC_T || (AHEAD && !AEM && !LGYM), "accumulated time: AHEAD structure, no row-major action windows, no lean gym outputs");
  constexpr int S = M::S, A = M::A, O = M::O;
  extern __shared__ __align__(16) unsigned char excenv_smem[];
  static_assert(NT == BLOCK || (!GENERAL && !AEM && !M::HAS_LUT), "wide workgroups: lean instantiations only (plain or with gym outputs)");
  constexpr bool ROW_BARRIER = NT > BLOCK;  // wide workgroups: the sixteen waves store every row together
  // GENERAL stays at one environment per lane. Round 4 tried two, each with its own property set (a second Ctx in registers:
  // every leaf may differ per environment, so none can stay in SGPRs — 195 registers, two waves per SIMD): 5.91 ... 6.27 ms for one,
  // 6.02 ... 6.06 for two (tools/general_path_cost.py, two sessions) — no gain, removed. What did help is compiling the gym
  // outputs' code out where none are asked for (STATES == -2): 0.569 -> 0.60 of the roof, the lean one-environment form's level.
  static_assert(!(GENERAL && V > 1), "per-environment property sets: one environment per lane");
  static_assert(GENERAL == (STATES < 0), "STATES -1 / -2 (general, with / without the gym outputs' code) and 0 / 1 (lean)");
  static_assert(!LGYM || (!GENERAL && !M::HAS_LUT && aem_shape_ok<T, V>()), "lean gym outputs: widest lean form, no look-up model");
  constexpr int NC = GENERAL ? V : 1;  // property sets per lane
  constexpr bool GYM = GENERAL && STATES == -1;
  static_assert(!AEM || (!GENERAL && !M::HAS_LUT && aem_shape_ok<T, V>() && (16 / (int)sizeof(T)) % A == 0),
                "row-major actions are fused into the widest lean instantiation only");
  const int64_t blk0 = (int64_t)blockIdx.x * (NT * V);  // first env of this workgroup
  const unsigned lane_env = threadIdx.x * V;
  const int64_t i0 = blk0 + lane_env;
  Ctx<T, M> cs[NC];
#pragma unroll
  for (int v = 0; v < NC; ++v) {
    load_ctx<GENERAL>(cs[v], ka.kp, (i0 + v < ka.B) ? i0 + v : 0, ka.dt, ka.env_tau, ka.adv_coef);
    cs[v].lin_stop = ka.lin_stop;
    cs[v].lin_div = T(ka.K - 1);
    cs[v].lin_last = ka.K - 1;
  }
  Ctx<T, M>& c = cs[0];  // what is the same for every environment of the lane (dead time, look-up tables: V == 1 there)
#define EXCENV_CX(v) cs[GENERAL ? (v) : 0]
  stage_lut<M, T>(c, ka.kp);
  if constexpr (M::HAS_LUT) c.lut_lds = LUT_LDS ? 1 : 0;  // == ka.kp.lut_lds (launch_lane_major picks the instantiation by it)
  // host guarantees B % V == 0; AEM: B % (64 V) == 0 — a wave is whole or absent (its lanes also fetch for each other)
  if (i0 >= ka.B) return;

  T st[V][S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    T tmp[V];
    load_v<T, V>(ka.state_in[j] + blk0 + lane_env, tmp);
#pragma unroll
    for (int v = 0; v < V; ++v) st[v][j] = tmp[v];
  }
  AheadAux<T> aux[V];
  if constexpr (AHEAD && M::IS_PMSM) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      aux[v].eps0 = st[v][2];
      aux[v].prev_clip[0] = st[v][0];
      aux[v].prev_clip[1] = st[v][1];
    }
  }
  // LGYM, the other models (pendulum_env.py:297-309, 381-390 and the like): control_state is a subset of the S state fields, so at
  // most NCM = S controls. Everything that depends on a reference only — sin / cos of a controlled angle's reference or the
  // normalised reference of any other field, and the (constant) truncated flag of its observation column — is computed once per
  // trajectory with the functions the general instantiation calls per row: same values, same bits.
  constexpr int NCM = (LGYM && !M::IS_PMSM) ? S : 1;
  T gp_a[V][NCM], gp_b[V][NCM];
  uint8_t gp_f[V][NCM];
  if constexpr (LGYM && !M::IS_PMSM) {
#pragma unroll
    for (int j = 0; j < NCM; ++j) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        gp_a[v][j] = gp_b[v][j] = T(0);
        gp_f[v][j] = 0;
      }
      if (j < ka.n_control) {
        const int f = ka.control_idx[j];
        T lo = c.smin[0], hi = c.smax[0];
        bool ang = false;
#pragma unroll
        for (int q = 0; q < S; ++q) {
          lo = (f == q) ? c.smin[q] : lo;
          hi = (f == q) ? c.smax[q] : hi;
          ang = ang || (is_angle_field<M>(q) && f == q);
        }
        T tmp[V];
        load_v<T, V>(ka.reference[j] + blk0 + lane_env, tmp);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const T nr = normalize(tmp[v], lo, hi);
          gp_f[v][j] = xabs(nr) > T(1);
          if (ang) sincos_t(tmp[v], gp_a[v][j], gp_b[v][j]);
          else gp_a[v][j] = nr;
        }
      }
    }
  }
  // ... and the control columns' share of a row's packed truncated flags (lane-major flag layout [row][B][TW]: the V * TW bytes
  // of a lane's environments are adjacent; byte v * TW + O + j is control column j of environment v), once per trajectory
  constexpr int GP_NW = (LGYM && !M::IS_PMSM) ? (V * (O + NCM) + 3) / 4 : 1;
  uint32_t gp_w[GP_NW];
  if constexpr (LGYM && !M::IS_PMSM && M::ID != EXCENV_FLUID_TANK) {
#pragma unroll
    for (int i = 0; i < GP_NW; ++i) gp_w[i] = 0u;
    dispatch_count<0, NCM>(ka.n_control, [&](auto tag) {
      constexpr int NC = decltype(tag)::value, TWc = O + NC;
#pragma unroll
      for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const int b = v * TWc + O + j;
          gp_w[b >> 2] |= (uint32_t)gp_f[v][j] << ((b & 3) * 8);
        }
      }
    });
  }
  // LGYM, PMSM: the references of the controlled fields among i_d (3), i_q (4), torque (5), per environment of the lane
  T g_id[V], g_iq[V], g_tq[V];
  bool has_id = false, has_iq = false, has_tq = false;
  if constexpr (LGYM && M::IS_PMSM) {
#pragma unroll
    for (int v = 0; v < V; ++v) g_id[v] = g_iq[v] = g_tq[v] = T(0);
#pragma unroll
    for (int j = 0; j < EXCENV_MAX_CONTROL; ++j) {
      if (j < ka.n_control) {
        const int f = ka.control_idx[j];
        T tmp[V];
        load_v<T, V>(ka.reference[j] + blk0 + lane_env, tmp);
        if (f == 3) has_id = true;
        if (f == 4) has_iq = true;
        if (f == 5) has_tq = true;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          g_id[v] = (f == 3) ? tmp[v] : g_id[v];
          g_iq[v] = (f == 4) ? tmp[v] : g_iq[v];
          g_tq[v] = (f == 5) ? tmp[v] : g_tq[v];
        }
      }
    }
  }
  const bool deadtime_on = (M::IS_PMSM) ? (c.P[M::P - 1] > T(0)) : false;
  // look-up models: the table values at each environment's current operating point, found once per solver step and used
  // for the torque of the saved row and for the first stage of the step that starts there
  T memo[V][6];
  if constexpr (M::HAS_LUT && !AHEAD) {
#pragma unroll
    for (int v = 0; v < V; ++v) M::lookup(st[v][3], st[v][4], c, memo[v]);
  }

  // reference-tracking columns: constant along the trajectory, loaded and normalised once (static register indices)
  T rref[NC][EXCENV_MAX_CONTROL], cref[NC][EXCENV_MAX_CONTROL];
  if constexpr (GENERAL) {
#pragma unroll
    for (int v = 0; v < NC; ++v) {
#pragma unroll
      for (int j = 0; j < EXCENV_MAX_CONTROL; ++j) {
        rref[v][j] = T(0);
        cref[v][j] = T(0);
        if (j < ka.n_control) {
          const int f = ka.control_idx[j];
          T lo = cs[v].smin[0], hi = cs[v].smax[0];
#pragma unroll
          for (int q = 1; q < S; ++q) {
            lo = (f == q) ? cs[v].smin[q] : lo;
            hi = (f == q) ? cs[v].smax[q] : hi;
          }
          rref[v][j] = ka.reference[j][i0 + v];
          cref[v][j] = normalize(rref[v][j], lo, hi);
        }
      }
    }
  }

  const int64_t N = ka.K * ka.substeps;
  // V > 1 implies env stride 1; for V == 1 the host has checked that 256 * stride * sizeof(T) < 2^31
  const T* a_blk = ka.actions + (int64_t)blockIdx.x * ka.a_wg;
  T* o_blk = ka.obs + (int64_t)blockIdx.x * ka.o_wg;
  const int64_t s_blk = (int64_t)blockIdx.x * ka.s_wg;
  const unsigned a_lane = (V == 1) ? threadIdx.x * (unsigned)ka.a_sb : lane_env;
  const unsigned o_lane = (V == 1) ? threadIdx.x * (unsigned)ka.o_sb : lane_env;
  const unsigned s_lane = (V == 1) ? threadIdx.x * (unsigned)ka.s_sb : lane_env;
  const bool with_states = (STATES < 0) ? (ka.straj[0] != nullptr) : (STATES != 0);

  // EXCENV_OPT_KEEP_CONSTANT_COLUMNS (include/excenv.h). omega_el is a constant of a PMSM trajectory (Pmsm::f only reads st[6]), so
  // every row of its state leaf and of observation column 2 (its normalised value) repeats row 0. The caller says that the buffers
  // still hold an earlier launch's rows: where row 0 of both columns is, bit for bit, what this launch would store there, all their
  // rows are, and the wave leaves the two columns alone — 8 of the 68 bytes per environment-step of a write-bound kernel. Decided once
  // per wave (one scalar: two scalar branches per row, no per-lane predicate); a wave in which any environment differs — one that was
  // reset or given another speed — writes everything, as a launch without the flag does. Not in the row-major-action form (AEM): its
  // counted wait needs every store of a row behind a window fill (NSTORE below). Not with the lean gym outputs or the accumulated-time
  // clock either: there the vote cost registers (fp64 gym outputs 254 -> 290) for launches that are not write-bound to begin with.
  constexpr bool KEEPC = M::IS_PMSM && !M::HAS_LUT && !GENERAL && !AEM && !LGYM && !ACC_T;
  constexpr int KC_OBS = 2, KC_LEAF = 6;  // Pmsm::observe: ob[2] = normalize(st[6])
  bool keep = false;
  if constexpr (KEEPC) {
    if (__builtin_expect(ka.keep_const != 0, 1)) {  // (launch.hpp: lane-major rows, environment stride 1); kept in line: steady state
      T kept_o[V], kept_s[V];
      load_v<T, V>(o_blk + KC_OBS * ka.o_sc + o_lane, kept_o);
      if (with_states) load_v<T, V>(ka.straj[KC_LEAF] + s_blk + s_lane, kept_s);
      bool same = true;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        // what save_row(0) stores into the two columns, through the calls it makes: the same values, the same bits (the dead-time rows
        // it puts into sv[0 .. 1] reach neither omega_el nor its observation column)
        T sv0[S], ob0[O];
#pragma unroll
        for (int j = 0; j < S; ++j) sv0[j] = st[v][j];
        if constexpr (AHEAD) M::post(sv0, c);
        M::observe(sv0, c, ob0);
        same = same & same_bits(kept_o[v], ob0[KC_OBS]);  // (& : no branch per environment)
        if (with_states) same = same & same_bits(kept_s[v], sv0[KC_LEAF]);
      }
      keep = __builtin_amdgcn_readfirstlane((int)(__builtin_amdgcn_ballot_w64(!same) == 0)) != 0;
      if constexpr (V == 1 && !ROW_BARRIER) {
        // rows that leave through LDS are stored by the workgroup's waves for each other: the vote is the workgroup's (whole
        // workgroups only take that path, sim_plan.hpp: every thread is here). The word used is free until row 0 is staged.
        if (ka.row_sync == 2) {
          unsigned* vote = reinterpret_cast<unsigned*>(excenv_smem);
          if (threadIdx.x == 0) *vote = 0u;
          __syncthreads();
          if (!keep && (threadIdx.x & 63u) == 0u) *vote = 1u;
          __syncthreads();
          keep = __builtin_amdgcn_readfirstlane(*vote) == 0u;
          __syncthreads();
        }
      }
    }
  }

  // ---- save row n: observation, (control columns), state leaves, (gym outputs); returns the saved state in sv ----
  auto save_row = [&](int64_t n, T (&sv)[V][S]) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
#pragma unroll
      for (int j = 0; j < S; ++j) sv[v][j] = st[v][j];
      if constexpr (AHEAD) {
        if constexpr (M::HAS_LUT) M::post_q(sv[v], c, memo[v]);
        else M::post(sv[v], EXCENV_CX(v));
        if constexpr (M::IS_PMSM) {  // pmsm_env.py:785-791
          if (deadtime_on) {
            sv[v][0] = aux[v].prev_clip[0];  // row 0: still the initial buffer (prev_clip starts as it)
            sv[v][1] = aux[v].prev_clip[1];
          } else {
            sv[v][0] = T(0);
            sv[v][1] = T(0);
          }
        }
      }
    }
    T ob[V][O];
#pragma unroll
    for (int v = 0; v < V; ++v) M::observe(sv[v], EXCENV_CX(v), ob[v]);
    T* orow = o_blk + n * ka.o_sk;
    // the waves of a workgroup store a row together: always in the wide-workgroup form; with one environment per lane (4-byte
    // stores, 256-byte runs per wave and stream) where the host asks for it — PMSM with per-environment properties at B = 2^22:
    // 6.29 -> 5.50 ms (0.567 -> 0.648 of the roof), the lean V = 1 form 6.34 -> 5.61
    bool direct = true;
    if constexpr (ROW_BARRIER) {
      __builtin_amdgcn_s_barrier();
    } else if constexpr (V == 1 && !M::HAS_LUT && !AEM) {
      // row_sync == 2 (lane-major arrays, whole workgroups, 16-byte aligned): the row goes through LDS — every lane leaves its
      // values as [stream][lane] words, one barrier, then the waves share the streams and store 16 bytes per lane: 1 KiB runs per
      // instruction instead of 256-byte ones, a quarter of the store instructions. Two buffers alternate, so the barrier of row
      // n + 1 is also the one that frees row n's buffer.
      if (ka.row_sync == 2) {
        constexpr int VE = 16 / (int)sizeof(T), CH = NT / (64 * VE), NW = NT / 64;
        const int OWr = O + (GENERAL ? ka.n_control : 0);
        const int NS = OWr + (with_states ? S : 0);
        T* buf = reinterpret_cast<T*>(excenv_smem) + (unsigned)(n & 1) * (unsigned)(NS * NT);
#pragma unroll
        for (int q = 0; q < O; ++q) buf[q * NT + threadIdx.x] = ob[0][q];
        if constexpr (GENERAL) {
#pragma unroll
          for (int j = 0; j < EXCENV_MAX_CONTROL; ++j)
            if (j < ka.n_control) buf[(O + j) * NT + threadIdx.x] = cref[0][j];
        }
        if (with_states) {
#pragma unroll
          for (int j = 0; j < S; ++j) buf[(OWr + j) * NT + threadIdx.x] = sv[0][j];
        }
        // this wave's LDS writes must have landed before it signals: gfx950 backs barriers off instead of waiting implicitly, and the
        // compiler adds no wait in front of the raw builtin (the disassembly showed ds_write ...; s_barrier). lgkmcnt only — a
        // __syncthreads() would also drain the trajectory stores still in flight (vmcnt), which is what this path must not do
#if !(EXCENV_FAULT & 2)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
        __builtin_amdgcn_s_barrier();
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const unsigned ln = threadIdx.x & 63u;
        for (int u = wv; u < NS * CH; u += NW) {
          const int q = u / CH;
          const unsigned e = (unsigned)(u % CH) * (64u * VE) + ln * VE;
          if constexpr (KEEPC) {
            if (keep && (q == KC_OBS || q == OWr + KC_LEAF)) continue;  // (no state leaves: q < OWr)
          }
          T tmp[VE];
          load_v<T, VE>(buf + q * NT + e, tmp);
          T* dst = (q < OWr) ? orow + q * ka.o_sc : ka.straj[q - OWr] + s_blk + n * ka.s_sk;
          store_stream<T, VE>(dst + e, tmp);
        }
        direct = false;
      } else if (ka.row_sync) {
        __builtin_amdgcn_s_barrier();
      }
    } else if constexpr (V == 1) {
      if (ka.row_sync) __builtin_amdgcn_s_barrier();
    }
    if (direct) {
#pragma unroll
      for (int q = 0; q < O; ++q) {
        if constexpr (KEEPC) {
          if (keep && q == KC_OBS) continue;
        }
        T tmp[V];
#pragma unroll
        for (int v = 0; v < V; ++v) tmp[v] = ob[v][q];
        store_stream<T, V>(orow + q * ka.o_sc + o_lane, tmp);
      }
      if constexpr (GENERAL) {
#pragma unroll
        for (int j = 0; j < EXCENV_MAX_CONTROL; ++j) {
          if (j < ka.n_control) {
            T tmp[V];
#pragma unroll
            for (int v = 0; v < V; ++v) tmp[v] = cref[v][j];
            store_v<T, V>(orow + (O + j) * ka.o_sc + o_lane, tmp);
          }
        }
      }
      if (with_states) {
#pragma unroll
        for (int j = 0; j < S; ++j) {
          if constexpr (KEEPC) {
            if (keep && j == KC_LEAF) continue;
          }
          T tmp[V];
#pragma unroll
          for (int v = 0; v < V; ++v) tmp[v] = sv[v][j];
          store_stream<T, V>(ka.straj[j] + s_blk + n * ka.s_sk + s_lane, tmp);
        }
      }
    }
    if constexpr (LGYM && !M::IS_PMSM) {  // generate_reward / generate_truncated / generate_terminated of the other models, V wide
      const int64_t e0 = blk0 + lane_env;
      T rew[V];
#pragma unroll
      for (int v = 0; v < V; ++v) rew[v] = T(0);
#pragma unroll
      for (int j = 0; j < NCM; ++j) {
        if (j < ka.n_control) {
          const int f = ka.control_idx[j];
          bool ang = false;
#pragma unroll
          for (int q = 0; q < S; ++q) ang = ang || (is_angle_field<M>(q) && f == q);
#pragma unroll
          for (int v = 0; v < V; ++v) {
            T x, lo, hi;
            pick_field<M, T>(sv[v], c, f, x, lo, hi);
            if (ang) {
              T sx, cx;
              sincos_t(x, sx, cx);
              const T ds = sx - gp_a[v][j], dc = cx - gp_b[v][j];
              rew[v] = rew[v] + -(ds * ds + dc * dc);
            } else {
              const T d = normalize(x, lo, hi) - gp_a[v][j];
              rew[v] = rew[v] + -(d * d);
            }
          }
        }
      }
      uint8_t fl[V];
      if constexpr (M::ID == EXCENV_FLUID_TANK) {  // fluid_tank_env.py:325-333: constants (TW = 1)
#pragma unroll
        for (int v = 0; v < V; ++v) fl[v] = 0;
        store_flags<V>(ka.truncated + n * ka.t_sk + e0, fl);
      } else {
        // |obs| > 1 per observation column + the control columns' constant flags: the V * TW bytes of the lane's environments are
        // adjacent in the row — ONE 16-byte store for pendulum [theta] instead of four 4-byte ones (round 5; the store
        // instructions of a gym launch were 2.0 ... 2.5 x the plain launch's for 1.2 ... 1.4 x its bytes)
        dispatch_count<0, NCM>(ka.n_control, [&](auto tag) {
          constexpr int NC = decltype(tag)::value, TWc = O + NC, NB = V * TWc, NW = (NB + 3) / 4;
          uint32_t w[NW];
#pragma unroll
          for (int i = 0; i < NW; ++i) w[i] = gp_w[i];
#pragma unroll
          for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int q = 0; q < O; ++q) {
              const int b = v * TWc + q;
              w[b >> 2] |= (xabs(ob[v][q]) > T(1)) ? (1u << ((b & 3) * 8)) : 0u;
            }
          }
          store_flag_bytes<NB>(ka.truncated + n * ka.t_sk + e0 * TWc, w);
        });
#pragma unroll
        for (int v = 0; v < V; ++v) fl[v] = rew[v] == T(0);  // generate_terminated: reward == 0
      }
      if (n > 0) {
        store_stream<T, V>(ka.reward + (n - 1) * ka.g_sk + e0, rew);
        store_flags<V>(ka.terminated + (n - 1) * ka.g_sk + e0, fl);
      }
    }
    if constexpr (LGYM && M::IS_PMSM) {  // the same outputs for the V environments of a lane: truncated row n, reward / terminated row n - 1
      T rew[V];
      uint8_t fl[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        rew[v] = pmsm_reward<M, T>(sv[v], c, has_id, g_id[v], has_iq, g_iq[v], has_tq, g_tq[v]);
        const T nd = normalize(sv[v][3], c.smin[3], c.smax[3]), nq = normalize(sv[v][4], c.smin[4], c.smax[4]);
        fl[v] = sqrt_exceeds_one(nd * nd + nq * nq);  // pmsm_env.py:972-983: sqrt(.) > 1 (devmath.hpp), terminated == truncated
      }
      const int64_t e0 = blk0 + lane_env;
      store_flags<V>(ka.truncated + n * ka.t_sk + e0, fl);
      if (n > 0) {
        store_stream<T, V>(ka.reward + (n - 1) * ka.g_sk + e0, rew);
        store_flags<V>(ka.terminated + (n - 1) * ka.g_sk + e0, fl);
      }
    }
    if constexpr (GYM) {  // core_env.py:490-531: truncated on every row, reward / terminated on rows 1..N (V == 1 here)
      if (ka.truncated != nullptr) {
        const int64_t e = i0;
        uint8_t* tr = ka.truncated + e * ka.t_sb + n * ka.t_sk;
        const bool tail = n > 0;
        T* rw = tail ? ka.reward + e * ka.g_sb + (n - 1) * ka.g_sk : nullptr;
        uint8_t* te = tail ? ka.terminated + e * ka.g_sb + (n - 1) * ka.g_sk : nullptr;
        gym_outputs<M, T>(sv[0], ob[0], c, ka.n_control, ka.control_idx, rref[0], rw, te, tr, ka.t_sc);
      }
    }
  };
  auto publish_last = [&](const T (&sv)[V][S]) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
      T tmp[V];
#pragma unroll
      for (int v = 0; v < V; ++v) tmp[v] = sv[v][j];
      store_v<T, V>(ka.last_state[j] + blk0 + lane_env, tmp);
    }
  };
  T sv[V][S];
  if (N == 0) {  // no action row exists (ka.actions may be NULL)
    save_row(0, sv);
    publish_last(sv);
    return;
  }

  T a0[A][V], a1[A][V];
  // (k, sub): action row and sub-step of solver step n; (kn, subn): those of step n + 1
  int64_t k = 0, kn = 0;
  int32_t sub = 0, subn = 0;
  // ---- AEM: the wave's action windows in LDS (see the comment above the kernel) ----
  constexpr int VW = 16 / (int)sizeof(T);  // elements per 16-byte piece
  constexpr int SP = AEM ? VW / A : 1;     // action rows per piece
  constexpr int NP = aem_np<M>();          // pieces per window
  constexpr int EPI = 64 / NP;             // environments (reader lanes) per load instruction
  static_assert(64 % NP == 0, "a load instruction covers whole windows");
  const unsigned wave = threadIdx.x / 64u, lane64 = threadIdx.x % 64u;
  const unsigned wave_off = AEM ? __builtin_amdgcn_readfirstlane(wave * (unsigned)(V * NP * AEM_BLOCK_BYTES)) : 0u;  // this wave's blocks
  const unsigned wave_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)excenv_smem + wave_off;  // as an LDS address
  // reader side: lane l's environment v sits in block (v, l / EPI) at window offset (l % EPI) * NP * 16
  const unsigned rd_lane = (lane64 / EPI) * AEM_BLOCK_BYTES + (lane64 % EPI) * (NP * 16u);
  // loader side: lane t serves reader lane slot t / NP of the instruction's EPI, piece t % NP
  const unsigned ld_piece = lane64 % NP;
  const uint64_t ld_lane_off = AEM ? ((uint64_t)(wave * 64u + lane64 / NP) * V) * (uint64_t)ka.a_sb : 0;  // elements, before (i, v)
  // pieces per environment row (host: K * A % VW == 0, and K * A < 2^23: the window bookkeeping below is unsigned 32-bit scalar
  // arithmetic — as int64_t every division by a power of two was a 64-bit shift with a sign fix-up, per slot and step)
  const int32_t n_pieces = AEM ? (int32_t)((ka.K * A) / VW) : 0;
  constexpr int NSTORE = O + ((STATES != 0) ? S : 0);   // trajectory stores per saved row: issued between a fill and its first read
  // Sector-aligned windows (round 5). A window is NP pieces = 64 bytes and one fabric request — if it does not straddle two
  // 64-byte sectors of memory. Rows of K * A * sizeof(T) bytes start on 16-byte boundaries only (PMSM, K = 100: 800 bytes, every
  // second environment starts in the middle of a sector), so windows counted from the row's first byte straddled for half of the
  // environments: 6.8e7 fabric reads where 5.2e7 would do, FETCH_SIZE 1.29 x the action bytes (round 4). Now the windows of an
  // environment are the SECTORS its row touches: with ph = (first piece of the row) mod NP, row piece j sits at position
  // (j + ph) % NP of window (j + ph) / NP, the first window holds NP - ph pieces (the lanes in front of it re-fetch the row's first
  // piece, never read), every further one is one aligned sector. ph depends on the environment only through its slot v of the lane
  // (the lanes' environments are V apart and V * pieces-per-row is a multiple of NP — else ph = 0 for everybody: the round-4
  // scheme), so each slot keeps its own wave-uniform window count and refills when ITS window ends.
  const bool aem_aligned = AEM && ((n_pieces * V) % NP) == 0;
  unsigned aem_ph[V];
  int32_t w_hi[V];  // highest window requested so far, per slot (wave-uniform)
#pragma unroll
  for (int v = 0; v < V; ++v) {
    aem_ph[v] = aem_aligned ? (unsigned)((((uintptr_t)a_blk >> 4) + (uint64_t)v * (uint64_t)(uint32_t)n_pieces) % NP) : 0u;
    w_hi[v] = -1;
  }
  auto dma_window = [&](int v, int32_t w) __attribute__((always_inline)) {  // v: compile-time constant at every call
    if constexpr (AEM) {
      int32_t pc = w * NP + (int32_t)ld_piece - (int32_t)aem_ph[v];
      pc = pc < 0 ? 0 : (pc < n_pieces ? pc : n_pieces - 1);  // in front of the row / behind it: a piece of the row again (never read)
      const T* lane_src = a_blk + ld_lane_off + (int64_t)pc * VW;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        // Inline assembly, not __builtin_amdgcn_global_load_lds: the compiler treats an LDS-direct load as a FLAT access and puts
        // `s_waitcnt vmcnt(0)` in front of every later LDS read — that would drain the trajectory stores once per step. Hidden
        // from it, the only wait is the counted one in load_action below. M0 = the LDS byte address of the block: declared as
        // clobbered, and the s_nop is the wait state gfx9-family parts need between an SALU write of M0 and an LDS-direct load
        // (the compiler's hazard recognizer emits the same s_nop behind the builtin; it does not look inside an asm string).
        // tests/test_isa_guards.py checks both in the disassembly of the built library.
        const T* src = lane_src + (uint64_t)(i * EPI * V + v) * (uint64_t)ka.a_sb;
        // (M0 is a reserved register: clang warns that it "may not be preserved"; listing it is what makes the compiler's own M0
        // initialisations — s_set_gpr_idx, its LDS-direct loads — see this statement as a redefinition)
        EXCENV_LDS_DIRECT_LOAD(src, wave_lds + (unsigned)(v * NP + i) * AEM_BLOCK_BYTES);
      }
    }
  };
  int32_t pc_j = -1;                       // the piece held in pc_reg (wave-uniform)
  T pc_reg[AEM ? V : 1][AEM ? VW : 1];     // a slot's current 16-byte piece: SP rows of A values
  bool fill_pending = false;               // a window was requested and no counted wait has run since
  auto load_action = [&](int64_t krow, T (&dst)[A][V]) __attribute__((always_inline)) {
    if constexpr (AEM) {
      // Once per PIECE (SP rows), not per row (round 5, second half): the slot's 16-byte piece is read from its LDS window into
      // registers (one ds_read_b128), the rows are picked out of the registers, and a window whose LAST piece has just been read is
      // re-requested right away — its fill has SP rows instead of one to land, no LDS read of the wave sits behind a fill in flight
      // for SP rows, and the bookkeeping (which window, which position, last piece or not: ~110 scalar instructions per wave-step
      // when it ran per row and slot) runs once per piece. Measured: neutral to -2 % against the row-wise form on every workload
      // (same buffers) — neither the bookkeeping, nor reads queued behind a fill, nor the fill's slack is what the small models lose
      // with row-major actions (DESIGN.md §4.1b has the list of what was ruled out). Kept for what it removes.
      const uint32_t kr = (uint32_t)krow;              // 0 <= krow < K < 2^23
      const int32_t j = (int32_t)(kr / (uint32_t)SP);  // the row's piece of its environment's row
      const unsigned rs = kr % (uint32_t)SP;           // the row inside that piece
      const bool newp = j != pc_j;
      // first piece after a fill was requested (at least one row, i.e. one saved row's stores, earlier): everything but the
      // trajectory stores issued since must be back (vmcnt retires in issue order: with at least NSTORE vector-memory instructions
      // behind the fill, vmcnt(NSTORE) waits for the fill and for nothing it need not — fills of other slots issued behind it only
      // make the wait stricter; FEWER than NSTORE behind it and the wait would prove nothing — tools/isa_guards.py counts them on
      // every path of the built code). expcnt(6) never blocks here (no exports) and marks the hand-written waits for that tool.
      // Wave-uniform.
      if (newp && fill_pending) asm volatile("s_waitcnt vmcnt(%0) expcnt(6)" ::"n"((NSTORE + (EXCENV_FAULT & 1)) < 63 ? (NSTORE + (EXCENV_FAULT & 1)) : 63) : "memory");
      if (newp) {
        fill_pending = false;
        pc_j = j;
        uint32_t last_mask = 0u;  // slots whose piece is the last of a window with a successor not yet requested
        int32_t w[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const uint32_t q = (uint32_t)j + aem_ph[v];
          w[v] = (int32_t)(q / (uint32_t)NP);
          const unsigned pos = q % (uint32_t)NP;
          load_v<T, VW>(reinterpret_cast<const T*>(excenv_smem + wave_off + (unsigned)(v * NP) * AEM_BLOCK_BYTES + rd_lane + pos * 16u), pc_reg[v]);
          // (w_hi: once per window, whatever the clamped tail of the trajectory repeats)
          if (pos == NP - 1 && w[v] + 1 > w_hi[v] && (w[v] + 1) * NP - (int32_t)aem_ph[v] < n_pieces) last_mask |= 1u << v;
        }
        if (last_mask != 0u) {  // those windows' LDS is dead once the reads above have returned -> request their successors into it
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int v = 0; v < V; ++v) {
            if ((last_mask >> v) & 1u) {
              dma_window(v, w[v] + 1);
              w_hi[v] = w[v] + 1;
            }
          }
          fill_pending = true;
        }
      }
      // the row out of the registers (rs is wave-uniform: SP - 1 selects per value)
#pragma unroll
      for (int v = 0; v < V; ++v) {
#pragma unroll
        for (int q = 0; q < A; ++q) {
          T val = pc_reg[v][q];
#pragma unroll
          for (int r = 1; r < SP; ++r) {
            const T alt = pc_reg[v][r * A + q];  // (a value, not an lvalue: a ternary between two lvalues becomes a pointer select -> scratch)
            val = (rs == (unsigned)r) ? alt : val;
          }
          dst[q][v] = val;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < A; ++q) load_v<T, V>(a_blk + krow * ka.a_sk + q * ka.a_sc + a_lane, dst[q]);
    }
  };
  // ACC_T: the clock, and the size of the step the last next_row() was for
  SimClock<T> clk;
  T dt_step = ka.dt;
  if constexpr (ACC_T) clk.init(ka.dt, acc_step, acc_end, (int)ka.K);
  auto advance = [&](const T (&cur)[A][V], const T (&nxt)[A][V], int64_t k, int64_t k1) __attribute__((always_inline)) {
    if constexpr (ACC_T) {  // the only step-size-dependent field of Ctx (adv_coef and lin_stop follow env_tau)
#pragma unroll
      for (int v = 0; v < NC; ++v) cs[v].dt = dt_step;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      T ac[A], an[A];
#pragma unroll
      for (int q = 0; q < A; ++q) {
        ac[q] = cur[q][v];
        an[q] = nxt[q][v];
      }
      if constexpr (AHEAD) {
        env_advance_raw<M, SOLVER>(st[v], ac, an, k, k1, EXCENV_CX(v), aux[v], M::HAS_LUT ? &memo[v] : nullptr);
      } else {
        env_step<M, SOLVER>(st[v], ac, EXCENV_CX(v), M::HAS_LUT ? &memo[v] : nullptr);
      }
    }
  };
  auto next_index = [&]() {
    kn = k;
    subn = sub + 1;
    if (subn == ka.substeps) { subn = 0; kn = k + 1; }
  };
  const int64_t klast = ka.K - 1;
  // The action row of the c_i == 1 stages of step n (clamped: always a valid row) and, in kn, the first row of step n + 1. ACC_T:
  // those two are the same row — the clock's t_prev of step n + 1 is t_next of step n (t_next <= t_end holds throughout) — so the
  // row prefetched for the c_i == 1 stage is the next step's first row, as on the other paths: the ping-pong and single-step loops
  // below stay as they are. The clock advances once per lane and step, not per environment; readfirstlane keeps the addressing scalar.
  auto next_row = [&]() __attribute__((always_inline)) -> int64_t {
    if constexpr (ACC_T) {
      kn = __builtin_amdgcn_readfirstlane(clk.row_next());
      dt_step = clk.step_size();
      clk.advance();
      return kn;
    } else {
      next_index();
      return (kn < klast) ? kn : klast;
    }
  };
  if constexpr (AEM) {  // the first window of every environment
#pragma unroll
    for (int v = 0; v < V; ++v) {
      dma_window(v, 0);
      w_hi[v] = 0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // once per trajectory (the initial state has arrived as well)
  }
  load_action(0, a0);
  if constexpr (AEM) {
    // A slot whose first window holds a single piece has re-requested it already, and the loop's first load_action follows without a
    // saved row in between: nothing would stand behind that fill for the counted wait to count (found by tools/isa_guards.py on the
    // piece-wise form; the row-wise form of rounds 4 - 5 had the same hole for one-row pieces — PMSM fp64 — and an action pointer that
    // is 16- but not 64-byte aligned). Once per trajectory: wait for it outright.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    fill_pending = false;
  }
  // Euler: the K loop unrolled by two with ping-pong action registers (2-step prefetch distance, 2x loop code). Measured (DESIGN.md
  // §6): +3.5 % Euler, -5 % Tsit5. Look-up models keep the single-step loop: twice the (large) look-up code does not fit the
  // instruction cache
  constexpr bool PINGPONG = SOLVER == EXCENV_EULER && !M::HAS_LUT;
  if constexpr (PINGPONG) {
    for (int64_t n = 0;; n += 2) {
      // even step: a0 holds action row k; the row of step n + 1 goes to a1 (clamped: always a valid row, so the load is
      // unconditional and its result needs no merge with an undefined value)
      int64_t k1 = next_row();
      load_action(k1, a1);
      save_row(n, sv);
      if (n == N) break;
      advance(a0, a1, k, k1);
      k = kn;
      sub = subn;
      // odd step: roles swapped
      k1 = next_row();
      load_action(k1, a0);
      save_row(n + 1, sv);
      if (n + 1 == N) break;
      advance(a1, a0, k, k1);
      k = kn;
      sub = subn;
    }
  } else {
    for (int64_t n = 0;; ++n) {
      // the row of step n + 1 is requested before row n is saved (clamped: always a valid row, so the load is unconditional);
      // it is first needed by the register rotation after the compute phase
      const int64_t k1 = next_row();
      load_action(k1, a1);
      save_row(n, sv);
      if (n == N) break;
      advance(a0, a1, k, k1);
#pragma unroll
      for (int q = 0; q < A; ++q)
#pragma unroll
        for (int v = 0; v < V; ++v) a0[q][v] = a1[q][v];
      k = kn;
      sub = subn;
    }
  }
  publish_last(sv);
#undef EXCENV_CX
