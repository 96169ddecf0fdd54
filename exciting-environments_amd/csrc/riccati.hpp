// Host side of excenv_lqr_backward (include/excenv.h): the shapes riccati_kernel<T, S, A> (riccati.hip) is
// instantiated for, what the entry refuses, and the algorithmic bytes of a call. No model: the matrices are the caller's.
#pragma once
#include <cmath>
#include <cstdio>
#include "launch.hpp"

namespace excenv {

constexpr const char* riccati_name() { return "riccati_kernel"; }
constexpr int RICCATI_BLOCK = 256;  // four waves, one environment per lane

int launch_riccati(int dtype, int64_t B, int64_t N, const excenv_lqr_t& call, hipStream_t stream);

// The (S, A) of the six models: fluid tank (1, 1), pendulum and mass-spring-damper (2, 1), cart-pole and acrobot (4, 1), PMSM (7, 2)
inline bool riccati_shape(int S, int A) { return (A == 1 && (S == 1 || S == 2 || S == 4)) || (S == 7 && A == 2); }

// What excenv_lqr_backward refuses: EXCENV_OK, or the code with the message in `msg`. NULL pointers first, then values.
inline int riccati_refusal(int dtype, int64_t B, int64_t N, const excenv_lqr_t* c, char* msg, size_t n) {
  const char* fn = "excenv_lqr_backward";
  auto null = [&](const char* what) { std::snprintf(msg, n, "%s: %s is NULL", fn, what); return EXCENV_ENULL; };
  if (!c) return null("call");
  if (!c->jac) return null("call->jac");
  if (!c->Q) return null("call->Q");
  if (!c->R) return null("call->R");
  if (!c->gain) return null("call->gain");
  if (dtype != EXCENV_F32 && dtype != EXCENV_F64) {
    std::snprintf(msg, n, "%s: dtype must be EXCENV_F32 (0) or EXCENV_F64 (1) (got %d)", fn, dtype);
    return EXCENV_EINVAL;
  }
  if (B < 0 || N < 0) {
    std::snprintf(msg, n, "%s: bad B=%lld or N=%lld", fn, (long long)B, (long long)N);
    return EXCENV_EINVAL;
  }
  if (!riccati_shape(c->n_state, c->n_action)) {
    std::snprintf(msg, n, "%s: no riccati_kernel for n_state=%d, n_action=%d: the shapes are (1, 1), (2, 1), (4, 1) and (7, 2)", fn,
                  c->n_state, c->n_action);
    return EXCENV_EUNSUPPORTED;
  }
  if (!(c->reg >= 0.0)) {
    std::snprintf(msg, n, "%s: call->reg must not be negative or NaN (got %g)", fn, c->reg);
    return EXCENV_EINVAL;
  }
  if (c->store_all != 0 && c->store_all != 1) {
    std::snprintf(msg, n, "%s: call->store_all must be 0 or 1 (got %d)", fn, c->store_all);
    return EXCENV_EINVAL;
  }
  if ((B + RICCATI_BLOCK - 1) / RICCATI_BLOCK >= ((int64_t)1 << 31)) {
    std::snprintf(msg, n, "%s: batch too large for one launch", fn);
    return EXCENV_EUNSUPPORTED;
  }
  const int64_t row = (int64_t)c->n_state * (c->n_state + c->n_action);
  if (c->jac_row_stride != 0 && c->jac_row_stride < row * B) {
    std::snprintf(msg, n, "%s: call->jac_row_stride must be 0 or at least S (S + A) B = %lld (got %lld)", fn, (long long)(row * B),
                  (long long)c->jac_row_stride);
    return EXCENV_EINVAL;
  }
  return EXCENV_OK;
}

inline int64_t riccati_bytes(int dtype, int S, int A, int time_invariant, int has_q, int has_r, int store_all, int has_ff) {
  if ((dtype != EXCENV_F32 && dtype != EXCENV_F64) || !riccati_shape(S, A)) return -1;
  const int64_t elem = dtype == EXCENV_F32 ? 4 : 8;
  int64_t n = time_invariant ? 0 : (int64_t)S * (S + A);
  if (has_q) n += S;
  if (has_r) n += A;
  if (store_all) n += (int64_t)A * S + (has_ff ? A : 0);
  return n * elem;
}

}  // namespace excenv
