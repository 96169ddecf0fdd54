// The Riccati recursion of finite-horizon LQR / the backward pass of iLQR on stored linearisations (excenv_lqr_backward,
// include/excenv.h). One environment per lane, RICCATI_BLOCK lanes a workgroup, one launch for the whole horizon:
// P, p and the running sums stay in registers across the rows, every access is one element per lane and coalesced along the batch
// (element accesses only: a 16-byte form would need a second code path with two or four environments a lane, and the chain is
// latency-bound, not bandwidth-bound). The loads of row n - 1 are issued before the arithmetic of row n where PREFETCH is set: every
// instantiation but (7, 2) in fp64, which takes 400 of a lane's 512 registers without a second Jacobian row set of 126. It needs no
// model: one instantiation per (S, A) and element type, every loop unrolled at compile time. The operation order is the header's
// block, so the numpy twin of the tests reproduces the bits. Plain C++: no atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "riccati.hpp"

namespace excenv {

template <typename T> struct RiccatiArgs {
  int64_t B, N, jac_row_stride;
  const T* jac;  // [N][S][S + A][B]
  const T* Q;    // [S][S]
  const T* Qf;   // [S][S] (Q where the call gave none)
  const T* R;    // [A][A]
  const T* q;    // [N + 1][S][B] or nullptr
  const T* r;    // [N][A][B] or nullptr
  T reg;
  int store_all;
  T* gain;       // [N or 1][A][S][B]
  T* ff;         // [N or 1][A][B] or nullptr
  T* P0;         // [S][S][B] or nullptr
  T* p0;         // [S][B] or nullptr
  T* dV;         // [2][B] or nullptr
  int32_t* n_bad;  // [B] or nullptr
};

template <typename T, int S, int A, bool PREFETCH>
__global__ void __launch_bounds__(RICCATI_BLOCK) riccati_kernel(const RiccatiArgs<T> ka) {
  constexpr int C = S + A;
  static_assert(A == 1 || A == 2, "the LDL^T solve is written out for one and two actions");
  const int64_t b = (int64_t)blockIdx.x * RICCATI_BLOCK + threadIdx.x;
  if (b >= ka.B) return;
  const int64_t B = ka.B, N = ka.N;
  const bool has_q = ka.q != nullptr, has_r = ka.r != nullptr;
  const T reg = ka.reg;

  T P[S][S], p[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
#pragma unroll
    for (int j = i; j < S; ++j) P[i][j] = P[j][i] = ka.Qf[i * S + j];
    p[i] = has_q ? ka.q[(N * S + i) * B + b] : T(0);
  }
  T dv0 = T(0), dv1 = T(0);
  int32_t bad = 0;

  T J[S][C];  // the Jacobian row set of the row under way (PREFETCH: of the next one, from the top of the loop body on)
  auto load = [&](int64_t n) __attribute__((always_inline)) {
    const T* at = ka.jac + n * ka.jac_row_stride + b;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int c = 0; c < C; ++c) J[i][c] = at[(int64_t)(i * C + c) * B];
  };
  if (PREFETCH && N > 0) load(N - 1);

  for (int64_t n = N - 1; n >= 0; --n) {
    T F[S][S], G[S][A], qn[S], rn[A];
    if (!PREFETCH) load(n);
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int j = 0; j < S; ++j) F[i][j] = J[i][j];
#pragma unroll
      for (int a = 0; a < A; ++a) G[i][a] = J[i][S + a];
    }
    if (PREFETCH && n > 0 && ka.jac_row_stride != 0) load(n - 1);
#pragma unroll
    for (int i = 0; i < S; ++i) qn[i] = has_q ? ka.q[(n * S + i) * B + b] : T(0);
#pragma unroll
    for (int a = 0; a < A; ++a) rn[a] = has_r ? ka.r[(n * A + a) * B + b] : T(0);

    // W = P F, Wb = P G
    T W[S][S], Wb[S][A];
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        T s = P[i][0] * F[0][j];
#pragma unroll
        for (int k = 1; k < S; ++k) s = xfma(P[i][k], F[k][j], s);
        W[i][j] = s;
      }
#pragma unroll
      for (int a = 0; a < A; ++a) {
        T s = P[i][0] * G[0][a];
#pragma unroll
        for (int k = 1; k < S; ++k) s = xfma(P[i][k], G[k][a], s);
        Wb[i][a] = s;
      }
    }
    // Qxx = Q + F^T W (upper triangle, into P: the old P is dead), Qux = G^T W, Quu = R + G^T Wb
    T Qux[A][S], Quu[A][A], Qx[S], Qu[A];
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int j = i; j < S; ++j) {
        T s = ka.Q[i * S + j];
#pragma unroll
        for (int k = 0; k < S; ++k) s = xfma(F[k][i], W[k][j], s);
        P[i][j] = s;
      }
      T s = qn[i];
#pragma unroll
      for (int k = 0; k < S; ++k) s = xfma(F[k][i], p[k], s);
      Qx[i] = s;
    }
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        T s = G[0][a] * W[0][j];
#pragma unroll
        for (int k = 1; k < S; ++k) s = xfma(G[k][a], W[k][j], s);
        Qux[a][j] = s;
      }
#pragma unroll
      for (int c = a; c < A; ++c) {
        T s = ka.R[a * A + c];
#pragma unroll
        for (int k = 0; k < S; ++k) s = xfma(G[k][a], Wb[k][c], s);
        Quu[a][c] = Quu[c][a] = s;
      }
      T s = rn[a];
#pragma unroll
      for (int k = 0; k < S; ++k) s = xfma(G[k][a], p[k], s);
      Qu[a] = s;
    }
    // (Quu + reg I) [K | k] = -[Qux | Qu] by LDL^T without square roots
    T Kg[A][S], kf[A];
    bool ok;
    if constexpr (A == 1) {
      const T d0 = Quu[0][0] + reg;
      ok = d0 > T(0);
#pragma unroll
      for (int j = 0; j < S; ++j) Kg[0][j] = -Qux[0][j] / d0;
      kf[0] = -Qu[0] / d0;
    } else {
      const T d0 = Quu[0][0] + reg;
      const T l = Quu[0][1] / d0;
      const T d1 = xfma(-l, Quu[0][1], Quu[1][1] + reg);
      ok = d0 > T(0) && d1 > T(0);
      auto solve = [&](T g0, T g1, T& x0, T& x1) __attribute__((always_inline)) {
        const T y1 = xfma(-l, g0, g1);
        x1 = y1 / d1;
        x0 = xfma(-l, x1, g0 / d0);
      };
#pragma unroll
      for (int j = 0; j < S; ++j) solve(-Qux[0][j], -Qux[1][j], Kg[0][j], Kg[1][j]);
      solve(-Qu[0], -Qu[1], kf[0], kf[1]);
    }
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
      for (int j = 0; j < S; ++j) Kg[a][j] = ok ? Kg[a][j] : T(0);
      kf[a] = ok ? kf[a] : T(0);
    }
    bad += ok ? 0 : 1;
    // P = Qxx + K^T Quu K + K^T Qux + Qux^T K, p = Qx + K^T Quu k + K^T Qu + Qux^T k (the unregularised Quu)
    T QK[A][S], Qk[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        T s = Quu[a][0] * Kg[0][j];
#pragma unroll
        for (int c = 1; c < A; ++c) s = xfma(Quu[a][c], Kg[c][j], s);
        QK[a][j] = s;
      }
      T s = Quu[a][0] * kf[0];
#pragma unroll
      for (int c = 1; c < A; ++c) s = xfma(Quu[a][c], kf[c], s);
      Qk[a] = s;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int j = i; j < S; ++j) {
        T s = P[i][j];
#pragma unroll
        for (int a = 0; a < A; ++a) s = xfma(Kg[a][i], QK[a][j], s);
#pragma unroll
        for (int a = 0; a < A; ++a) s = xfma(Kg[a][i], Qux[a][j], s);
#pragma unroll
        for (int a = 0; a < A; ++a) s = xfma(Qux[a][i], Kg[a][j], s);
        P[i][j] = P[j][i] = s;
      }
      T s = Qx[i];
#pragma unroll
      for (int a = 0; a < A; ++a) s = xfma(Kg[a][i], Qk[a], s);
#pragma unroll
      for (int a = 0; a < A; ++a) s = xfma(Kg[a][i], Qu[a], s);
#pragma unroll
      for (int a = 0; a < A; ++a) s = xfma(Qux[a][i], kf[a], s);
      p[i] = s;
    }
    T h = kf[0] * Qk[0];
#pragma unroll
    for (int a = 1; a < A; ++a) h = xfma(kf[a], Qk[a], h);
#pragma unroll
    for (int a = 0; a < A; ++a) dv0 = xfma(kf[a], Qu[a], dv0);
    dv1 = dv1 + T(0.5) * h;

    if (ka.store_all || n == 0) {
      const int64_t row = ka.store_all ? n : 0;
#pragma unroll
      for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int j = 0; j < S; ++j) ka.gain[((row * A + a) * S + j) * B + b] = Kg[a][j];
        if (ka.ff) ka.ff[(row * A + a) * B + b] = kf[a];
      }
    }
  }

  if (ka.P0) {
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) ka.P0[(int64_t)(i * S + j) * B + b] = P[i][j];
  }
  if (ka.p0) {
#pragma unroll
    for (int i = 0; i < S; ++i) ka.p0[(int64_t)i * B + b] = p[i];
  }
  if (ka.dV) {
    ka.dV[b] = dv0;
    ka.dV[B + b] = dv1;
  }
  if (ka.n_bad) ka.n_bad[b] = bad;
}

template <typename T, int S, int A> static int launch_riccati_t(int64_t B, int64_t N, const excenv_lqr_t& c, hipStream_t stream) {
  RiccatiArgs<T> ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.N = N;
  ka.jac_row_stride = c.jac_row_stride;
  ka.jac = (const T*)c.jac;
  ka.Q = (const T*)c.Q;
  ka.Qf = (const T*)(c.Qf ? c.Qf : c.Q);
  ka.R = (const T*)c.R;
  ka.q = (const T*)c.q;
  ka.r = (const T*)c.r;
  ka.reg = (T)c.reg;
  ka.store_all = c.store_all;
  ka.gain = (T*)c.gain;
  ka.ff = (T*)c.ff;
  ka.P0 = (T*)c.P0;
  ka.p0 = (T*)c.p0;
  ka.dV = (T*)c.dV;
  ka.n_bad = c.n_bad;
  // a second Jacobian row set in flight wherever it fits next to P, W and the first: all but (7, 2) in fp64
  constexpr bool PREFETCH = S * (S + A) * sizeof(T) <= 63 * 4;
  const int64_t blocks = (B + RICCATI_BLOCK - 1) / RICCATI_BLOCK;
  hipLaunchKernelGGL((riccati_kernel<T, S, A, PREFETCH>), dim3((unsigned)blocks), dim3(RICCATI_BLOCK), 0, stream, ka);
  g_last_launch = riccati_name();
  return check_launch("excenv_lqr_backward");
}

template <typename T> static int launch_riccati_shape(int64_t B, int64_t N, const excenv_lqr_t& c, hipStream_t stream) {
  if (c.n_action == 1) {
    if (c.n_state == 1) return launch_riccati_t<T, 1, 1>(B, N, c, stream);
    if (c.n_state == 2) return launch_riccati_t<T, 2, 1>(B, N, c, stream);
    if (c.n_state == 4) return launch_riccati_t<T, 4, 1>(B, N, c, stream);
  }
  if (c.n_state == 7 && c.n_action == 2) return launch_riccati_t<T, 7, 2>(B, N, c, stream);
  set_error("excenv_lqr_backward: no riccati_kernel for n_state=%d, n_action=%d", c.n_state, c.n_action);
  return EXCENV_EUNSUPPORTED;
}

int launch_riccati(int dtype, int64_t B, int64_t N, const excenv_lqr_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_riccati_shape<float>(B, N, call, stream) : launch_riccati_shape<double>(B, N, call, stream);
}

}  // namespace excenv
