// The solver clock of EXCENV_SEM_AHEAD_ACCUMULATED_T (include/excenv.h): the oracle's restatement of diffrax's fixed-step loop
// (the CPU oracle's oracle_body.inc, ORACLE_SEM_AHEAD_ACCUMULATED_T; unpinned: diffrax itself is not part of any test). (t_prev, t_next) are
// carried in the working precision T; a step's size is t_next - t_prev; the action row a stage reads is int(t / action_stepsize) at
// the stage's time, clamped to [0, K - 1]: t_prev for the first stage and every stage with c_i < 1, t_next for stages with c_i == 1.
// Host-and-device and free of HIP when compiled for the host, like sim_plan.hpp: the host C++ compiler builds it alone
// (tests/test_sim_clock.py). Every value is the same for every environment of a call (wave-uniform).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EXCENV_HD __host__ __device__
#else
#define EXCENV_HD
#endif

namespace excenv {

template <typename T> struct SimClock {
  T a_step;  // T(obs_stepsize * substeps): the action step
  T t_end;   // T(obs_stepsize * substeps * K), folded in double like the oracle
  T t_prev, t_next;
  int klast;  // K - 1 (the host bounds K below 2^30)

  // diffrax's _clip_to_end: a t_next within this of t1 is snapped to it
  static constexpr T tol() { return sizeof(T) == 8 ? T(1e-10) : T(1e-6); }

  EXCENV_HD void init(T obs_stepsize, T action_step, T end, int K) {
    a_step = action_step;
    t_end = end;
    klast = K - 1;
    t_prev = T(0);
    t_next = obs_stepsize;  // t0 + dt0
    if (t_next > t_end - tol()) t_next = t_end;
  }
  // int(t / action_stepsize) clamped to a valid row. IEEE division on purpose: the row flips exactly where the quotient rounds
  // across an integer, so a reciprocal or a fast division would pick other rows.
  EXCENV_HD int row(T t) const {
    const int k = (int)(t / a_step);
    return k < 0 ? 0 : (k > klast ? klast : k);
  }
  EXCENV_HD int row_prev() const { return row(t_prev); }  // stage 1 and every stage with c_i < 1
  EXCENV_HD int row_next() const { return row(t_next); }  // stages with c_i == 1
  EXCENV_HD T step_size() const { return t_next - t_prev; }
  // ConstantStepSize: (t_next, t_next + (t_next - t_prev)), t_next clipped to the end. t_next <= t_end always holds, so the new
  // t_prev is the old t_next: the row of the next step's first stage is this step's row_next().
  EXCENV_HD void advance() {
    const T t_new = t_next + (t_next - t_prev);
    t_prev = t_next < t_end ? t_next : t_end;
    t_next = t_new > t_end - tol() ? t_end : t_new;
  }
};

}  // namespace excenv

#undef EXCENV_HD
