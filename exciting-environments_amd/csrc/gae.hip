// Generalised advantage estimation on lane-major rows (excenv_gae, include/excenv.h): the backward scan
//   delta[n] = fma(g, nt ? value[n + 1] : 0, reward[n]) - value[n];  carry = nt ? fma(gl, carry, delta[n]) : delta[n]
// per environment, with reset[n] cutting the scan (advantage 0, returns value[n], carry 0). One environment per lane, GAE_BLOCK lanes
// a workgroup, every access one element per lane and coalesced along the batch. The loads of row n and its delta do not depend on
// the carry: GAE_DEPTH rows of loads stay in flight in a register ring ahead of the scan, whose serial chain is one fma and one
// select per row. It needs no model: two instantiations, one per element type. Plain C++: no atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.hpp"

namespace excenv {

template <typename T> struct GaeArgs {
  int64_t B, K;
  T g, gl;  // (T)gamma and (T)(g * (T)lambda)
  const T* reward;        // [K][B]
  const T* value;         // [K + 1][B]
  const uint8_t* term;    // [K][B] or nullptr
  const uint8_t* reset;   // [K][B] or nullptr
  T* adv;                 // [K][B]
  T* ret;                 // [K][B] or nullptr
};

template <typename T> __global__ void __launch_bounds__(GAE_BLOCK) gae_kernel(const GaeArgs<T> ka) {
  constexpr int D = GAE_DEPTH;
  const int64_t b = (int64_t)blockIdx.x * GAE_BLOCK + threadIdx.x;
  if (b >= ka.B) return;
  const int64_t B = ka.B, K = ka.K;
  const T g = ka.g, gl = ka.gl;
  const bool has_term = ka.term != nullptr, has_reset = ka.reset != nullptr, has_ret = ka.ret != nullptr;

  // slot s of the ring holds row n0 - s of the rows n0 .. n0 - D + 1 under way; rows below 0 are not loaded
  T rw[D], vl[D];
  uint8_t tm[D], rs[D];
  auto load = [&](int64_t n, int s) __attribute__((always_inline)) {
    rw[s] = T(0), vl[s] = T(0), tm[s] = 0, rs[s] = 0;
    if (n >= 0) {
      const int64_t at = n * B + b;
      rw[s] = ka.reward[at];
      vl[s] = ka.value[at];
      if (has_term) tm[s] = ka.term[at];
      if (has_reset) rs[s] = ka.reset[at];
    }
  };
#pragma unroll
  for (int s = 0; s < D; ++s) load(K - 1 - s, s);
  T next = ka.value[K * B + b];  // value[n + 1]
  T carry = T(0);
  for (int64_t n0 = K - 1; n0 >= 0; n0 -= D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      const int64_t n = n0 - s;
      if (n >= 0) {
        const T r = rw[s], v = vl[s];
        const bool nt = tm[s] == 0, cut = rs[s] != 0;
        load(n - D, s);
        const T boot = nt ? next : T(0);
        const T delta = xfma(g, boot, r) - v;
        const T run = nt ? xfma(gl, carry, delta) : delta;
        carry = cut ? T(0) : run;
        const int64_t at = n * B + b;
        ka.adv[at] = carry;
        if (has_ret) ka.ret[at] = cut ? v : carry + v;
        next = v;
      }
    }
  }
}

template <typename T> static int launch_gae_t(int64_t B, int64_t K, const excenv_gae_t& c, hipStream_t stream) {
  GaeArgs<T> ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.K = K;
  ka.g = (T)c.gamma;
  ka.gl = (T)(ka.g * (T)c.lambda);
  ka.reward = (const T*)c.reward;
  ka.value = (const T*)c.value;
  ka.term = c.terminated;
  ka.reset = c.reset;
  ka.adv = (T*)c.advantage;
  ka.ret = (T*)c.returns;
  const int64_t blocks = (B + GAE_BLOCK - 1) / GAE_BLOCK;
  if (blocks >= ((int64_t)1 << 31)) { set_error("excenv_gae: batch too large for one launch"); return EXCENV_EUNSUPPORTED; }
  hipLaunchKernelGGL((gae_kernel<T>), dim3((unsigned)blocks), dim3(GAE_BLOCK), 0, stream, ka);
  g_last_launch = gae_name();
  return check_launch("excenv_gae");
}

int launch_gae(int dtype, int64_t B, int64_t K, const excenv_gae_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_gae_t<float>(B, K, call, stream) : launch_gae_t<double>(B, K, call, stream);
}

}  // namespace excenv
