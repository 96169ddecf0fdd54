// The clipped PPO objective of a diagonal Gaussian policy on lane-major rows (excenv_gaussian_logp, excenv_ppo_loss,
// excenv_ppo_loss_grad, include/excenv.h). Three streams over the same sample tiles, EXCENV_PPO_TILE consecutive
// environments of one row: lane l of a 256-lane workgroup holds the samples 4 l .. 4 l + 3 of the tile, one 16-byte access an array in
// fp32 and two in fp64 where B % 4 == 0 and the arrays are 16-byte aligned, four element accesses otherwise (the same samples on the
// same lanes, so the sums do not depend on the path). A workgroup owns a contiguous run of tiles (ppo_groups, policy.hpp) and keeps
// the loads of the next tile in flight while it works on this one.
//   gaussian_logp_kernel : logp = logp_const - 0.5 sum z^2 by fused multiply-adds, no transcendental
//   ppo_loss_kernel      : the sums of the contract block, every term in T, added in fp64 per lane; the lanes of a workgroup by a fixed
//                          tree into one partial set of the workspace; ppo_loss_reduce_kernel adds the sets the same way. No atomics.
//   ppo_loss_grad_kernel : grad_mean [K][A][B] and grad_value [K][B], selects for the reset mask and the clip
// Plain C++: no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <initializer_list>
#include "launch.hpp"

namespace excenv {

template <typename T> struct PpoArgs {
  int64_t B, K, tiles_per_row, tiles, groups;
  const T *mean, *sample, *inv_std, *logp_const;  // [K][A][B] twice, [A], [1]
  const T *logp_old, *adv, *value, *ret;          // [K][B]; value / ret may be nullptr
  const T *adv_norm, *grad_scale;                 // [2] or nullptr
  const uint8_t* reset;                           // [K][B] or nullptr
  T lo, hi;                                       // (T)(1 - clip_eps), (T)(1 + clip_eps)
  int vec, reset_word;                            // 16-byte accesses of the arrays of T; 4-byte accesses of the flag bytes
  T* logp;                                        // (out) gaussian_logp_kernel
  double* partial;                                // (out) ppo_loss_kernel: [groups][PPO_SLOTS]
  T *grad_mean, *grad_value;                      // (out) ppo_loss_grad_kernel; either may be nullptr
};

enum PpoMode { PPO_LOGP = 0, PPO_LOSS = 1, PPO_GRAD = 2 };

__device__ __forceinline__ float xexp(float x) { return expf(x); }
__device__ __forceinline__ double xexp(double x) { return exp(x); }

// four consecutive elements at p + at: cnt of them exist (the others read as 0); vec: at is a multiple of four elements and 16-byte aligned
template <typename T> __device__ __forceinline__ void load4(const T* __restrict__ p, int64_t at, int cnt, bool vec, T (&o)[PPO_LANE]) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + at);
      o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
      const double2 u = *reinterpret_cast<const double2*>(p + at), v = *reinterpret_cast<const double2*>(p + at + 2);
      o[0] = u.x, o[1] = u.y, o[2] = v.x, o[3] = v.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPO_LANE; ++j) o[j] = j < cnt ? p[at + j] : T(0);
  }
}
template <typename T> __device__ __forceinline__ void store4(T* __restrict__ p, int64_t at, int cnt, bool vec, const T (&o)[PPO_LANE]) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<float4*>(p + at) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      *reinterpret_cast<double2*>(p + at) = make_double2(o[0], o[1]);
      *reinterpret_cast<double2*>(p + at + 2) = make_double2(o[2], o[3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPO_LANE; ++j)
      if (j < cnt) p[at + j] = o[j];
  }
}

// What a lane holds of one tile
template <typename T, int A, int MODE> struct PpoTile {
  int cnt;  // samples of this lane that exist: 0 .. 4
  int64_t at;  // n * B + b
  int64_t atq;  // n * A * B + b
  T m[A][PPO_LANE], x[A][PPO_LANE];
  T lp[PPO_LANE], ad[PPO_LANE], vl[PPO_LANE], rt[PPO_LANE];
  uint32_t rs;  // the four flag bytes, the first one lowest
};

template <typename T, int A, int MODE>
__device__ __forceinline__ void ppo_load(const PpoArgs<T>& ka, int64_t tile, PpoTile<T, A, MODE>& w) {
  const int64_t n = tile / ka.tiles_per_row, bt = tile - n * ka.tiles_per_row;
  const int64_t b = bt * EXCENV_PPO_TILE + (int64_t)threadIdx.x * PPO_LANE;
  const int64_t left = ka.B - b;
  w.cnt = left <= 0 ? 0 : left < PPO_LANE ? (int)left : PPO_LANE;
  w.at = n * ka.B + b;
  w.atq = n * A * ka.B + b;
  w.rs = 0;
  if (w.cnt == 0) return;
  const bool vec = ka.vec != 0;
#pragma unroll
  for (int q = 0; q < A; ++q) {
    load4(ka.mean, w.atq + q * ka.B, w.cnt, vec, w.m[q]);
    load4(ka.sample, w.atq + q * ka.B, w.cnt, vec, w.x[q]);
  }
  if constexpr (MODE != PPO_LOGP) {
    load4(ka.logp_old, w.at, w.cnt, vec, w.lp);
    load4(ka.adv, w.at, w.cnt, vec, w.ad);
    if (ka.value) {
      load4(ka.value, w.at, w.cnt, vec, w.vl);
      load4(ka.ret, w.at, w.cnt, vec, w.rt);
    }
    if (ka.reset) {
      if (ka.reset_word) {
        w.rs = *reinterpret_cast<const uint32_t*>(ka.reset + w.at);
      } else {
#pragma unroll
        for (int j = 0; j < PPO_LANE; ++j)
          if (j < w.cnt) w.rs |= (uint32_t)ka.reset[w.at + j] << (8 * j);
      }
    }
  }
}

// the sum of v over the workgroup's 256 lanes, in lane 0 (fixed tree: shuffles within a wave, then waves 0..3 in order)
__device__ __forceinline__ double ppo_block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // the slots of the sum before this one have been read
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return threadIdx.x == 0 ? ((lds[0] + lds[1]) + lds[2]) + lds[3] : 0.0;
}

template <typename T, int A, int MODE> __device__ __forceinline__ void ppo_body(const PpoArgs<T>& ka) {
  const int64_t g = blockIdx.x;
  const int64_t per = ka.tiles / ka.groups, rem = ka.tiles % ka.groups;
  const int64_t first = g * per + (g < rem ? g : rem), last = first + per + (g < rem ? 1 : 0);
  const bool vec = ka.vec != 0;
  T is[A];
#pragma unroll
  for (int q = 0; q < A; ++q) is[q] = ka.inv_std[q];
  const T lc = ka.logp_const[0];
  T shift = T(0), scale = T(1), w = T(0), wv = T(0);
  const bool norm = MODE != PPO_LOGP && ka.adv_norm != nullptr, has_value = MODE != PPO_LOGP && ka.value != nullptr;
  if (norm) shift = ka.adv_norm[0], scale = ka.adv_norm[1];
  if constexpr (MODE == PPO_GRAD) w = ka.grad_scale[0], wv = ka.grad_scale[1];
  double acc[PPO_SLOTS];
#pragma unroll
  for (int i = 0; i < PPO_SLOTS; ++i) acc[i] = 0.0;

  PpoTile<T, A, MODE> cur, nxt;
  if (first < last) ppo_load<T, A, MODE>(ka, first, cur);
  for (int64_t t = first; t < last; ++t) {
    nxt.cnt = 0;
    if (t + 1 < last) ppo_load<T, A, MODE>(ka, t + 1, nxt);  // in flight while this tile is worked on
    if (cur.cnt > 0) {
      T out_lp[PPO_LANE], gm[A][PPO_LANE], gv[PPO_LANE];
#pragma unroll
      for (int j = 0; j < PPO_LANE; ++j) {
        T z[A];
        T lp = lc;
#pragma unroll
        for (int q = 0; q < A; ++q) {
          z[q] = (cur.x[q][j] - cur.m[q][j]) * is[q];
          lp = xfma(T(-0.5) * z[q], z[q], lp);
        }
        out_lp[j] = lp;
        if constexpr (MODE != PPO_LOGP) {
          const T d = lp - cur.lp[j];
          const T r = xexp(d);
          const T a = norm ? (cur.ad[j] - shift) * scale : cur.ad[j];
          const T s1 = r * a;
          const T rl = r < ka.lo ? ka.lo : r;
          const T rc = rl > ka.hi ? ka.hi : rl;
          const T s2 = rc * a;
          const bool active = !(s2 < s1);
          const bool valid = j < cur.cnt && ((cur.rs >> (8 * j)) & 0xffu) == 0;
          const T dv = has_value ? cur.vl[j] - cur.rt[j] : T(0);
          if constexpr (MODE == PPO_LOSS) {
            const T surr = s2 < s1 ? s2 : s1;
            const T g0 = active ? -s1 : T(0);
            acc[0] += valid ? 1.0 : 0.0;
            acc[1] += valid ? (double)surr : 0.0;
            acc[2] += valid ? (double)(dv * dv) : 0.0;
            acc[3] += valid ? (double)((r - T(1)) - d) : 0.0;
            acc[4] += valid && (r < ka.lo || r > ka.hi) ? 1.0 : 0.0;
#pragma unroll
            for (int q = 0; q < A; ++q) acc[EXCENV_PPO_STATS + q] += valid ? (double)(g0 * (z[q] * z[q] - T(1))) : 0.0;
          } else {
            const T gl = active ? -s1 * w : T(0);
#pragma unroll
            for (int q = 0; q < A; ++q) gm[q][j] = valid ? gl * z[q] * is[q] : T(0);
            gv[j] = valid ? wv * dv : T(0);
          }
        }
      }
      if constexpr (MODE == PPO_LOGP) store4(ka.logp, cur.at, cur.cnt, vec, out_lp);
      if constexpr (MODE == PPO_GRAD) {
        if (ka.grad_mean) {
#pragma unroll
          for (int q = 0; q < A; ++q) store4(ka.grad_mean, cur.atq + q * ka.B, cur.cnt, vec, gm[q]);
        }
        if (ka.grad_value) store4(ka.grad_value, cur.at, cur.cnt, vec, gv);
      }
    }
    cur = nxt;
  }
  if constexpr (MODE == PPO_LOSS) {
    __shared__ double lds[PPO_BLOCK / 64];
#pragma unroll
    for (int i = 0; i < PPO_SLOTS; ++i) {
      const double s = ppo_block_sum(acc[i], lds);
      if (threadIdx.x == 0) ka.partial[g * PPO_SLOTS + i] = s;
    }
  }
}

template <typename T, int A> __global__ void __launch_bounds__(PPO_BLOCK) gaussian_logp_kernel(const PpoArgs<T> ka) {
  ppo_body<T, A, PPO_LOGP>(ka);
}
template <typename T, int A> __global__ void __launch_bounds__(PPO_BLOCK) ppo_loss_kernel(const PpoArgs<T> ka) {
  ppo_body<T, A, PPO_LOSS>(ka);
}
template <typename T, int A> __global__ void __launch_bounds__(PPO_BLOCK) ppo_loss_grad_kernel(const PpoArgs<T> ka) {
  ppo_body<T, A, PPO_GRAD>(ka);
}

// stats[i] = the sum of the `groups` partial sets: lane l adds the sets l, l + 256, .. in ascending order, then the fixed tree
__global__ void __launch_bounds__(PPO_BLOCK) ppo_loss_reduce_kernel(const double* __restrict__ partial, int64_t groups, int n_stats,
                                                                     double* __restrict__ stats) {
  __shared__ double lds[PPO_BLOCK / 64];
  for (int i = 0; i < n_stats; ++i) {
    double v = 0.0;
    for (int64_t s = threadIdx.x; s < groups; s += PPO_BLOCK) v += partial[s * PPO_SLOTS + i];
    const double sum = ppo_block_sum(v, lds);
    if (threadIdx.x == 0) stats[i] = sum;
  }
}

template <typename T> static bool ppo_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p && !aligned16(p)) return false;
  return true;
}

template <typename T> static void ppo_shape(PpoArgs<T>& ka, int64_t B, int64_t K, int32_t max_groups) {
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.K = K;
  ka.tiles_per_row = (B + EXCENV_PPO_TILE - 1) / EXCENV_PPO_TILE;
  ka.tiles = ppo_tiles(B, K);
  ka.groups = ppo_groups(B, K, max_groups);
}

template <typename T> static int launch_gaussian_logp_t(int64_t B, int64_t K, const excenv_gaussian_logp_t& c, hipStream_t stream) {
  PpoArgs<T> ka;
  ppo_shape(ka, B, K, 0);
  ka.mean = (const T*)c.mean;
  ka.sample = (const T*)c.sample;
  ka.inv_std = (const T*)c.inv_std;
  ka.logp_const = (const T*)c.logp_const;
  ka.logp = (T*)c.logp;
  ka.vec = (B % PPO_LANE == 0 && ppo_aligned<T>({c.mean, c.sample, c.logp})) ? 1 : 0;
  const dim3 grid((unsigned)ka.groups), block(PPO_BLOCK);
  if (c.n_actions == 1) hipLaunchKernelGGL((gaussian_logp_kernel<T, 1>), grid, block, 0, stream, ka);
  else hipLaunchKernelGGL((gaussian_logp_kernel<T, 2>), grid, block, 0, stream, ka);
  g_last_launch = gaussian_logp_name();
  return check_launch("excenv_gaussian_logp");
}

template <typename T> static int launch_ppo_loss_t(bool grad, int64_t B, int64_t K, const excenv_ppo_loss_t& c, hipStream_t stream) {
  PpoArgs<T> ka;
  ppo_shape(ka, B, K, grad ? 0 : c.max_groups);
  ka.mean = (const T*)c.mean;
  ka.sample = (const T*)c.sample;
  ka.inv_std = (const T*)c.inv_std;
  ka.logp_const = (const T*)c.logp_const;
  ka.logp_old = (const T*)c.logp_old;
  ka.adv = (const T*)c.advantage;
  ka.value = (const T*)c.value;
  ka.ret = (const T*)c.returns;
  ka.adv_norm = (const T*)c.adv_norm;
  ka.reset = c.reset;
  ka.lo = (T)(1.0 - c.clip_eps);
  ka.hi = (T)(1.0 + c.clip_eps);
  ka.reset_word = (B % PPO_LANE == 0 && (reinterpret_cast<uintptr_t>(c.reset) & 3u) == 0) ? 1 : 0;
  bool vec = B % PPO_LANE == 0 && ppo_aligned<T>({c.mean, c.sample, c.logp_old, c.advantage, c.value, c.returns});
  const dim3 grid((unsigned)ka.groups), block(PPO_BLOCK);
  if (grad) {
    ka.grad_scale = (const T*)c.grad_scale;
    ka.grad_mean = (T*)c.grad_mean;
    ka.grad_value = (T*)c.grad_value;
    ka.vec = (vec && ppo_aligned<T>({c.grad_mean, c.grad_value})) ? 1 : 0;
    if (c.n_actions == 1) hipLaunchKernelGGL((ppo_loss_grad_kernel<T, 1>), grid, block, 0, stream, ka);
    else hipLaunchKernelGGL((ppo_loss_grad_kernel<T, 2>), grid, block, 0, stream, ka);
    g_last_launch = ppo_loss_grad_name();
    return check_launch("excenv_ppo_loss_grad");
  }
  ka.vec = vec ? 1 : 0;
  ka.partial = (double*)c.workspace;
  if (c.n_actions == 1) hipLaunchKernelGGL((ppo_loss_kernel<T, 1>), grid, block, 0, stream, ka);
  else hipLaunchKernelGGL((ppo_loss_kernel<T, 2>), grid, block, 0, stream, ka);
  hipLaunchKernelGGL(ppo_loss_reduce_kernel, dim3(1), block, 0, stream, (const double*)ka.partial, ka.groups,
                     EXCENV_PPO_STATS + c.n_actions, c.stats);
  g_last_launch = ppo_loss_name();
  return check_launch("excenv_ppo_loss");
}

int launch_gaussian_logp(int dtype, int64_t B, int64_t K, const excenv_gaussian_logp_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_gaussian_logp_t<float>(B, K, call, stream) : launch_gaussian_logp_t<double>(B, K, call, stream);
}

int launch_ppo_loss(bool grad, int dtype, int64_t B, int64_t K, const excenv_ppo_loss_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_ppo_loss_t<float>(grad, B, K, call, stream) : launch_ppo_loss_t<double>(grad, B, K, call, stream);
}

}  // namespace excenv
