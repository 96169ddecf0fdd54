// Rollout statistics on lane-major rows (excenv_row_moments, excenv_episode_stats, include/excenv.h).
//   row_moments_kernel          : the masked column sums S1[c], S2[c] and the count of the contract block. ppo_loss_kernel's launch shape:
//                                 tiles of EXCENV_PPO_TILE consecutive environments of one row, lane l of a 256-lane workgroup holds the
//                                 samples 4 l .. 4 l + 3, one 16-byte access a column in fp32 and two in fp64 where B % 4 == 0 and x is
//                                 16-byte aligned, four element accesses otherwise (the same samples on the same lanes). A workgroup owns a
//                                 contiguous run of tiles and keeps the loads of the next tile in flight. The columns go in passes of 4, 2
//                                 and 1 so that a pass's sums are registers of a compile-time count; a column's order of summation does not
//                                 depend on its pass.
//   episode_stats_kernel        : gae_kernel's shape run forwards: one environment per lane, EPISODE_DEPTH rows of loads in a register ring
//                                 ahead of the scan, whose serial chain is one fp64 add and the selects.
//   rollout_stats_reduce_kernel : adds (and, for the last two slots of the episode statistics, compares) the partial sets of either.
// Per-lane fp64 values go through a fixed tree (shuffles within a wave, then the waves 0 .. 3 in order through LDS) into one partial set
// per workgroup. Plain C++: no atomics, no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.hpp"

namespace excenv {
namespace {

constexpr int SL = PPO_LANE;  // consecutive samples of a lane

enum StatOp { STAT_SUM = 0, STAT_MIN = 1, STAT_MAX = 2 };

// v OP w with the comparisons of the contract: the incoming value w replaces v only where it compares below (above) it
template <int OP> __device__ __forceinline__ double stat_join(double v, double w) {
  if constexpr (OP == STAT_SUM) return v + w;
  else if constexpr (OP == STAT_MIN) return w < v ? w : v;
  else return w > v ? w : v;
}

// v joined over the workgroup's 256 lanes, in lane 0 (fixed tree: shuffles within a wave, then waves 0 .. 3 in order)
template <int OP> __device__ __forceinline__ double stat_block(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = stat_join<OP>(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // the slots of the value before this one have been read
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return threadIdx.x == 0 ? stat_join<OP>(stat_join<OP>(stat_join<OP>(lds[0], lds[1]), lds[2]), lds[3]) : 0.0;
}

// four consecutive elements at p + at: cnt of them exist (the others read as 0); vec: at is a multiple of four elements and 16-byte aligned
template <typename T> __device__ __forceinline__ void stat_load4(const T* __restrict__ p, int64_t at, int cnt, bool vec, T (&o)[SL]) {
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
    for (int j = 0; j < SL; ++j) o[j] = j < cnt ? p[at + j] : T(0);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- the column moments
template <typename T> struct MomentsArgs {
  int64_t B, N, tiles_per_row, tiles, groups;
  int C;
  const T* x;           // [N][C][B]
  const uint8_t* mask;  // [N][B] or nullptr
  const double* shift;  // [C] or nullptr
  int vec, mask_word;   // 16-byte accesses of x; 4-byte accesses of the mask bytes
  double* partial;      // (out) [groups][1 + 2 C]
};

// What a lane holds of one tile and CB columns
template <typename T, int CB> struct MomentsTile {
  int cnt;      // samples of this lane that exist: 0 .. 4
  uint32_t ms;  // the four mask bytes, the first one lowest
  T x[CB][SL];
};

template <typename T, int CB>
__device__ __forceinline__ void moments_load(const MomentsArgs<T>& ka, int64_t tile, int c0, MomentsTile<T, CB>& w) {
  const int64_t n = tile / ka.tiles_per_row, bt = tile - n * ka.tiles_per_row;
  const int64_t b = bt * EXCENV_PPO_TILE + (int64_t)threadIdx.x * SL;
  const int64_t left = ka.B - b;
  w.cnt = left <= 0 ? 0 : left < SL ? (int)left : SL;
  w.ms = 0;
  if (w.cnt == 0) return;
  const bool vec = ka.vec != 0;
  const int64_t atq = (n * ka.C + c0) * ka.B + b;
#pragma unroll
  for (int q = 0; q < CB; ++q) stat_load4(ka.x, atq + q * ka.B, w.cnt, vec, w.x[q]);
  if (ka.mask) {
    const int64_t at = n * ka.B + b;
    if (ka.mask_word) {
      w.ms = *reinterpret_cast<const uint32_t*>(ka.mask + at);
    } else {
#pragma unroll
      for (int j = 0; j < SL; ++j)
        if (j < w.cnt) w.ms |= (uint32_t)ka.mask[at + j] << (8 * j);
    }
  }
}

// the columns c0 .. c0 + CB - 1 over the workgroup's tiles -> their slots of the workgroup's partial set (and the count with c0 == 0)
template <typename T, int CB>
__device__ __forceinline__ void moments_pass(const MomentsArgs<T>& ka, int64_t first, int64_t last, int c0, double* lds) {
  double sh[CB], s1[CB], s2[CB], cnt = 0.0;
#pragma unroll
  for (int q = 0; q < CB; ++q) sh[q] = ka.shift ? ka.shift[c0 + q] : 0.0, s1[q] = 0.0, s2[q] = 0.0;
  MomentsTile<T, CB> cur, nxt;
  cur.cnt = 0;
  if (first < last) moments_load<T, CB>(ka, first, c0, cur);
  for (int64_t t = first; t < last; ++t) {
    nxt.cnt = 0;
    if (t + 1 < last) moments_load<T, CB>(ka, t + 1, c0, nxt);  // in flight while this tile is added
    if (cur.cnt > 0) {
#pragma unroll
      for (int j = 0; j < SL; ++j) {
        const bool valid = j < cur.cnt && ((cur.ms >> (8 * j)) & 0xffu) == 0;
        cnt += valid ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < CB; ++q) {
          const double d = (double)cur.x[q][j] - sh[q];
          const double dd = d * d;
          s1[q] += valid ? d : 0.0;
          s2[q] += valid ? dd : 0.0;
        }
      }
    }
    cur = nxt;
  }
  double* out = ka.partial + (int64_t)blockIdx.x * (1 + 2 * ka.C);
  if (c0 == 0) {
    const double s = stat_block<STAT_SUM>(cnt, lds);
    if (threadIdx.x == 0) out[0] = s;
  }
#pragma unroll
  for (int q = 0; q < CB; ++q) {
    const double a = stat_block<STAT_SUM>(s1[q], lds), b = stat_block<STAT_SUM>(s2[q], lds);
    if (threadIdx.x == 0) out[1 + c0 + q] = a, out[1 + ka.C + c0 + q] = b;
  }
}

template <typename T> __global__ void __launch_bounds__(STATS_BLOCK) row_moments_kernel(const MomentsArgs<T> ka) {
  __shared__ double lds[STATS_BLOCK / 64];
  const int64_t g = blockIdx.x;
  const int64_t per = ka.tiles / ka.groups, rem = ka.tiles % ka.groups;
  const int64_t first = g * per + (g < rem ? g : rem), last = first + per + (g < rem ? 1 : 0);
  int c0 = 0;
  for (; c0 + 4 <= ka.C; c0 += 4) moments_pass<T, 4>(ka, first, last, c0, lds);
  if (c0 + 2 <= ka.C) {
    moments_pass<T, 2>(ka, first, last, c0, lds);
    c0 += 2;
  }
  if (c0 < ka.C) moments_pass<T, 1>(ka, first, last, c0, lds);
}

// ---------------------------------------------------------------------------------------------------------------- the episode scan
template <typename T> struct EpisodeArgs {
  int64_t B, K;
  const T* reward;         // [K][B]
  const uint8_t* reset;    // [K][B]
  const double* ret_in;    // [B] or nullptr
  const int32_t* steps_in; // [B] or nullptr
  double* completed;       // (out) [K][B] or nullptr
  double* ret_out;         // (out) [B] or nullptr
  int32_t* steps_out;      // (out) [B] or nullptr
  double* partial;         // (out) [blocks][EXCENV_EPISODE_STATS]
};

template <typename T> __global__ void __launch_bounds__(STATS_BLOCK) episode_stats_kernel(const EpisodeArgs<T> ka) {
  constexpr int D = EPISODE_DEPTH;
  __shared__ double lds[STATS_BLOCK / 64];
  const int64_t B = ka.B, K = ka.K;
  const int64_t b = (int64_t)blockIdx.x * STATS_BLOCK + threadIdx.x;
  const bool live = b < B;  // the lanes past the batch load and store nothing and join the tree with the neutral values
  const bool has_completed = ka.completed != nullptr;

  // slot s of the ring holds row n0 + s of the rows n0 .. n0 + D - 1 under way; rows from K on are not loaded
  T rw[D];
  uint8_t rs[D];
  auto load = [&](int64_t n, int s) __attribute__((always_inline)) {
    rw[s] = T(0), rs[s] = 0;
    if (live && n < K) {
      const int64_t at = n * B + b;
      rw[s] = ka.reward[at];
      rs[s] = ka.reset[at];
    }
  };
#pragma unroll
  for (int s = 0; s < D; ++s) load(s, s);
  double ret = (live && ka.ret_in) ? ka.ret_in[b] : 0.0;
  int32_t len = (live && ka.steps_in) ? ka.steps_in[b] : 0;
  double cnt = 0.0, sr = 0.0, srr = 0.0, sl = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
  for (int64_t n0 = 0; n0 < K; n0 += D) {
#pragma unroll
    for (int s = 0; s < D; ++s) {
      const int64_t n = n0 + s;
      if (n < K) {
        const double r = (double)rw[s];
        const bool cut = rs[s] != 0;
        load(n + D, s);
        const bool emit = cut && len > 0;
        const double done = emit ? ret : 0.0;  // off the chain: what the episode that ends here adds
        const double sq = ret * ret;
        cnt += emit ? 1.0 : 0.0;
        sr += done;
        srr += emit ? sq : 0.0;
        sl += emit ? (double)len : 0.0;
        mn = (emit && ret < mn) ? ret : mn;
        mx = (emit && ret > mx) ? ret : mx;
        if (has_completed && live) ka.completed[n * B + b] = done;
        const double run = ret + r;
        ret = cut ? 0.0 : run;
        len = cut ? 0 : len + 1;
      }
    }
  }
  if (live) {
    if (ka.ret_out) ka.ret_out[b] = ret;
    if (ka.steps_out) ka.steps_out[b] = len;
  }
  double* out = ka.partial + (int64_t)blockIdx.x * EXCENV_EPISODE_STATS;
  const double t0 = stat_block<STAT_SUM>(cnt, lds), t1 = stat_block<STAT_SUM>(sr, lds), t2 = stat_block<STAT_SUM>(srr, lds);
  const double t3 = stat_block<STAT_SUM>(sl, lds), t4 = stat_block<STAT_MIN>(mn, lds), t5 = stat_block<STAT_MAX>(mx, lds);
  if (threadIdx.x == 0) out[0] = t0, out[1] = t1, out[2] = t2, out[3] = t3, out[4] = t4, out[5] = t5;
}

// ---------------------------------------------------------------------------------------------------------------- the second launch
// stats[i] = the `sets` partial sets joined: lane l takes the sets l, l + 256, .. in ascending order, then the fixed tree. The first
// n_sum slots are sums; minmax: one minimum and one maximum follow them
__global__ void __launch_bounds__(STATS_BLOCK) rollout_stats_reduce_kernel(const double* __restrict__ partial, int64_t sets, int n_sum,
                                                                           int minmax, double* __restrict__ stats) {
  __shared__ double lds[STATS_BLOCK / 64];
  const int stride = n_sum + (minmax ? 2 : 0);
  for (int i = 0; i < n_sum; ++i) {
    double v = 0.0;
    for (int64_t s = threadIdx.x; s < sets; s += STATS_BLOCK) v += partial[s * stride + i];
    const double sum = stat_block<STAT_SUM>(v, lds);
    if (threadIdx.x == 0) stats[i] = sum;
  }
  if (minmax) {
    double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    for (int64_t s = threadIdx.x; s < sets; s += STATS_BLOCK) {
      lo = stat_join<STAT_MIN>(lo, partial[s * stride + n_sum]);
      hi = stat_join<STAT_MAX>(hi, partial[s * stride + n_sum + 1]);
    }
    const double a = stat_block<STAT_MIN>(lo, lds), b = stat_block<STAT_MAX>(hi, lds);
    if (threadIdx.x == 0) stats[n_sum] = a, stats[n_sum + 1] = b;
  }
}

template <typename T> static int launch_row_moments_t(int64_t B, int64_t N, const excenv_row_moments_t& c, hipStream_t stream) {
  MomentsArgs<T> ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.N = N;
  ka.C = c.n_columns;
  ka.tiles_per_row = (B + EXCENV_PPO_TILE - 1) / EXCENV_PPO_TILE;
  ka.tiles = ppo_tiles(B, N);
  ka.groups = ppo_groups(B, N, c.max_groups);
  ka.x = (const T*)c.x;
  ka.mask = c.mask;
  ka.shift = c.shift;
  ka.vec = (B % SL == 0 && aligned16(c.x)) ? 1 : 0;
  ka.mask_word = (B % SL == 0 && (reinterpret_cast<uintptr_t>(c.mask) & 3u) == 0) ? 1 : 0;
  ka.partial = (double*)c.workspace;
  hipLaunchKernelGGL((row_moments_kernel<T>), dim3((unsigned)ka.groups), dim3(STATS_BLOCK), 0, stream, ka);
  hipLaunchKernelGGL(rollout_stats_reduce_kernel, dim3(1), dim3(STATS_BLOCK), 0, stream, (const double*)ka.partial, ka.groups,
                     1 + 2 * ka.C, 0, c.stats);
  g_last_launch = row_moments_name();
  return check_launch("excenv_row_moments");
}

template <typename T> static int launch_episode_stats_t(int64_t B, int64_t K, const excenv_episode_stats_t& c, hipStream_t stream) {
  EpisodeArgs<T> ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.K = K;
  ka.reward = (const T*)c.reward;
  ka.reset = c.reset;
  ka.ret_in = c.return_in;
  ka.steps_in = c.steps_in;
  ka.completed = c.completed;
  ka.ret_out = c.return_out;
  ka.steps_out = c.steps_out;
  ka.partial = (double*)c.workspace;
  const int64_t blocks = episode_stats_groups(B);
  hipLaunchKernelGGL((episode_stats_kernel<T>), dim3((unsigned)blocks), dim3(STATS_BLOCK), 0, stream, ka);
  hipLaunchKernelGGL(rollout_stats_reduce_kernel, dim3(1), dim3(STATS_BLOCK), 0, stream, (const double*)ka.partial, blocks,
                     EXCENV_EPISODE_STATS - 2, 1, c.stats);
  g_last_launch = episode_stats_name();
  return check_launch("excenv_episode_stats");
}

int launch_row_moments(int dtype, int64_t B, int64_t N, const excenv_row_moments_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_row_moments_t<float>(B, N, call, stream) : launch_row_moments_t<double>(B, N, call, stream);
}

int launch_episode_stats(int dtype, int64_t B, int64_t K, const excenv_episode_stats_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_episode_stats_t<float>(B, K, call, stream) : launch_episode_stats_t<double>(B, K, call, stream);
}

}  // namespace excenv
