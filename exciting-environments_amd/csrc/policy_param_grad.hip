// The parameter gradient of a policy rollout on the matrix cores (excenv_policy_param_grad, include/excenv.h):
//   grad_params = sum over b < B, k < K of (d mlp / d params)(obs[k * substeps][.][b])^T grad_raw[k][.][b]
// It needs no model: two instantiations, one per element type. v_mfma_f32_16x16x4_f32 and v_mfma_f64_16x16x4_f64 have the same
// shape (lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]; only the result's rows differ), so one tile routine
// serves both: an f32 MFMA is bit for bit a k-ordered fmaf chain.
//   A sample tile is 64 consecutive environments of one action row, read 64 wide from the lane-major arrays (tail lanes load zeros:
// their d^L is zero, so is everything they add). It lives in dynamic LDS as rows [unit][sample] of PARAM_GRAD_LDS_STRIDE elements
// (policy.hpp): x^0, every hidden x^l, d^L and a row of ones. Per tile, with four waves:
//   1. forward, l = 1 .. L - 1: x^l = act(W_l x^{l-1} + b_l). A = W_l from global memory, B = x^{l-1} from LDS, C starts at b_l: the
//      forward kernel's own chain (bias, then the inputs in ascending order). Wave w owns the samples 16 w .. 16 w + 15.
//   2. weight gradient, l = L .. 1: dW_l += d^l (x^{l-1})^T with the 64 samples as the k index, 16 MFMAs per 16 x 16 output tile; the
//      row of ones behind x^{l-1} makes db_l one more column. The output tiles of all layers are dealt round the waves (tile id =
//      4 slot + wave) and stay in registers, PARAM_GRAD_SLOTS per wave, across all of the workgroup's sample tiles.
//   3. transposed, l = L .. 2: d^{l-1} = (W_l^T d^l) * act'(x^{l-1}), written over x^{l-1} in place behind a barrier (product 2 of
//      layer l was the last reader of x^{l-1}). Wave w owns its 16 samples again.
// Dimensions that are no multiple of 16 or 4 are zero-filled by a select on the operand behind a clamped index: nothing is read out
// of bounds. After EXCENV_PARAM_GRAD_CHAIN samples at the most the owning lane adds an accumulator into the workgroup's own fp64 slot
// of the workspace (the first flush stores: no zeroing pass); policy_param_grad_reduce_kernel adds the slots in ascending order.
// Which tiles a workgroup owns is a function of (B, K, max_groups) alone. No atomics, no inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_policy_vjp.hpp"

namespace excenv {

template <typename T> struct ParamGradArgs {
  int64_t B, nbt, tiles;  // nbt = ceil(B / 64) tiles per action row
  int64_t obs_krow;       // elements between the observation rows of two action rows: substeps * OW * B
  int32_t groups, n_params;
  int32_t n_layers, activation;
  int32_t widths[EXCENV_POLICY_MAX_LAYERS + 1];
  const T* obs;     // [K * substeps + 1][OW][B]
  const T* graw;    // [K][A][B]
  double* partial;  // [groups][n_params]
};

template <typename T> struct Mma;
template <> struct Mma<float> {
  typedef float V __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ V mma(float a, float b, V c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};
template <> struct Mma<double> {
  typedef double V __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ V mma(double a, double b, V c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }  // (not the f32 map)
};

extern __shared__ __attribute__((aligned(16))) unsigned char param_grad_lds[];

// one value per layer l = 1 .. 4, picked by compares
struct Tab4 {
  int a, b, c, d;
  __device__ __forceinline__ int at(int l) const { return l == 1 ? a : l == 2 ? b : l == 3 ? c : d; }
};
static_assert(EXCENV_POLICY_MAX_LAYERS == 4, "Tab4");

template <typename T>
__global__ void __launch_bounds__(PARAM_GRAD_BLOCK) policy_param_grad_kernel(const ParamGradArgs<T> ka, const T* __restrict__ params) {
  using M = Mma<T>;
  using V = typename M::V;
  constexpr int LD = PARAM_GRAD_LDS_STRIDE, NS = PARAM_GRAD_SLOTS, TILE = PARAM_GRAD_TILE;
  constexpr int NPRE = (EXCENV_POLICY_MAX_INPUT + EXCENV_MAX_ACTION + 3) / 4;  // staged rows per wave
  constexpr int FLUSH_TILES = EXCENV_PARAM_GRAD_CHAIN / TILE;
  static_assert(EXCENV_PARAM_GRAD_CHAIN % TILE == 0 && EXCENV_PARAM_GRAD_CHAIN <= 4096, "whole tiles, within the measured range of the f32 chain");
  T* const lds = reinterpret_cast<T*>(param_grad_lds);
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = ka.n_layers, activation = ka.activation;

  // per layer l, in scalar registers (no arrays: nothing here may be indexed at run time): inputs, outputs, where W_l starts, the LDS
  // rows of x^{l-1} and of d^l (x^l's own rows; d^L sits where an x^L would), the output tiles of the layers before l
  const int w0 = ka.widths[0], w1 = ka.widths[1], w2 = L >= 2 ? ka.widths[2] : 1, w3 = L >= 3 ? ka.widths[3] : 1, w4 = L >= 4 ? ka.widths[4] : 1;
  const Tab4 nin{w0, L >= 2 ? w1 : 1, L >= 3 ? w2 : 1, L >= 4 ? w3 : 1}, dl{w1, w2, w3, w4};
  const int sz1 = dl.a * (nin.a + 1), sz2 = L >= 2 ? dl.b * (nin.b + 1) : 0, sz3 = L >= 3 ? dl.c * (nin.c + 1) : 0;
  const Tab4 poff{0, sz1, sz1 + sz2, sz1 + sz2 + sz3};
  const Tab4 xrow{0, nin.a, nin.a + nin.b, nin.a + nin.b + nin.c};
  const Tab4 drow{xrow.b, xrow.c, xrow.d, xrow.d + nin.d};
  auto out_tiles = [](int d, int ni) { return ((d + 15) >> 4) * ((ni + 16) >> 4); };
  const int nt1 = out_tiles(dl.a, nin.a), nt2 = L >= 2 ? out_tiles(dl.b, nin.b) : 0, nt3 = L >= 3 ? out_tiles(dl.c, nin.c) : 0,
            nt4 = L >= 4 ? out_tiles(dl.d, nin.d) : 0;
  const Tab4 cum{0, nt1, nt1 + nt2, nt1 + nt2 + nt3};  // the output tiles of layers 1 .. l - 1
  const int n_out = cum.d + nt4;
  const int OW = w0, A = dl.at(L), graw_row = drow.at(L), ones_row = graw_row + A;

  // the wave's output tiles of the weight products: slot t holds tile 4 t + wave as layer | row tile << 4 | column tile << 8 (0: none)
  int sinfo[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) {
    const int id = 4 * t + wave;
    sinfo[t] = 0;
    if (id < n_out) {
      const int l = id < cum.b ? 1 : id < cum.c ? 2 : id < cum.d ? 3 : 4;
      const int local = id - cum.at(l);
      const int nit = (nin.at(l) + 16) >> 4;
      const int jt = local / nit;
      sinfo[t] = l | (jt << 4) | ((local - jt * nit) << 8);
    }
  }

  const int64_t g = blockIdx.x;
  const int64_t tq = ka.tiles / ka.groups, tr = ka.tiles % ka.groups;
  const int64_t t_lo = g * tq + (g < tr ? g : tr), t_hi = (g + 1) * tq + (g + 1 < tr ? g + 1 : tr);

  // the rows of tile t this wave stages: row wave + 4 r of x^0 (OW rows) followed by d^L (A rows)
  auto load_tile = [&](int64_t t, T (&pre)[NPRE]) __attribute__((always_inline)) {
    const int64_t k = t / ka.nbt;
    const int64_t b = (t - k * ka.nbt) * TILE + lane;
    const bool live = b < ka.B;
#pragma unroll
    for (int r = 0; r < NPRE; ++r) {
      const int row = wave + 4 * r;
      pre[r] = T(0);
      if (row < OW) {
        if (live) pre[r] = ka.obs[k * ka.obs_krow + (int64_t)row * ka.B + b];
      } else if (row < OW + A) {
        if (live) pre[r] = ka.graw[(k * A + (row - OW)) * ka.B + b];
      }
    }
  };
  auto store_tile = [&](const T (&pre)[NPRE]) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < NPRE; ++r) {
      const int row = wave + 4 * r;
      if (row < OW) lds[row * LD + lane] = pre[r];
      else if (row < OW + A) lds[(graw_row + (row - OW)) * LD + lane] = pre[r];
    }
  };

  V acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = V{T(0), T(0), T(0), T(0)};
  if (tid < TILE) lds[ones_row * LD + tid] = T(1);
  double* const slot = ka.partial + g * ka.n_params;
  bool first = true;
  int since = 0;
  const int scol = 16 * wave + lr;  // the sample column of this lane in products 1 and 3

  T pre[NPRE];
  load_tile(t_lo, pre);
  for (int64_t t = t_lo; t < t_hi; ++t) {
    store_tile(pre);
    __syncthreads();
    if (t + 1 < t_hi) load_tile(t + 1, pre);

    // ---- 1. forward: the hidden layers
    for (int l = 1; l < L; ++l) {
      const int ni = nin.at(l), d = dl.at(l), off = poff.at(l);
      const T* xin = lds + xrow.at(l) * LD + scol;
      T* xout = lds + drow.at(l) * LD + scol;
      const T* bias = params + off + d * ni;
      for (int j0 = 0; j0 < d; j0 += 16) {
        V c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + M::row(lane, r);
          c[r] = bias[j < d ? j : d - 1];
        }
        const bool jok = j0 + lr < d;
        const T* w = params + off + (jok ? j0 + lr : d - 1) * ni;
        for (int i0 = 0; i0 < ni; i0 += 4) {
          const int i = i0 + lq;
          const bool iok = i < ni;
          const int ic = iok ? i : ni - 1;
          const T a = w[ic], b = xin[ic * LD];
          c = M::mma((iok && jok) ? a : T(0), iok ? b : T(0), c);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + M::row(lane, r);
          if (j < d) xout[j * LD] = policy_act(c[r], activation);
        }
      }
      __syncthreads();
    }

    // ---- 2. and 3., the layers backwards
    for (int l = L; l >= 1; --l) {
      const int ni = nin.at(l), d = dl.at(l), off = poff.at(l), xr = xrow.at(l), dr = drow.at(l);
      // 2. dW_l += d^l (x^{l-1}, 1)^T over the 64 samples
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int info = sinfo[s];
        if ((info & 15) == l) {
          const int j = 16 * ((info >> 4) & 15) + lr, i = 16 * (info >> 8) + lr;
          const bool jok = j < d, iok = i <= ni;
          const T* ap = lds + (dr + (jok ? j : d - 1)) * LD + lq;
          const T* bp = lds + (i < ni ? xr + i : ones_row) * LD + lq;
          V c = acc[s];
#pragma unroll 4
          for (int s0 = 0; s0 < TILE; s0 += 4) {
            const T a = ap[s0], b = bp[s0];
            c = M::mma(jok ? a : T(0), iok ? b : T(0), c);
          }
          acc[s] = c;
        }
      }
      if (l > 1) {
        __syncthreads();
        // 3. d^{l-1} = (W_l^T d^l) * act'(x^{l-1}) over x^{l-1}
        const T* dp = lds + dr * LD + scol;
        T* xp = lds + xr * LD + scol;
        for (int i0 = 0; i0 < ni; i0 += 16) {
          V c = V{T(0), T(0), T(0), T(0)};
          const bool iok = i0 + lr < ni;
          const T* w = params + off + (iok ? i0 + lr : ni - 1);
          for (int j0 = 0; j0 < d; j0 += 4) {
            const int j = j0 + lq;
            const bool jok = j < d;
            const int jc = jok ? j : d - 1;
            const T a = w[jc * ni], b = dp[jc * LD];
            c = M::mma((iok && jok) ? a : T(0), jok ? b : T(0), c);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + M::row(lane, r);
            if (i < ni) xp[i * LD] = policy_act_vjp(c[r], xp[i * LD], activation);
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();  // the tile has been read: the next one may be stored

    // ---- bounded chains: the accumulators go to the workgroup's fp64 slot
    if (++since == FLUSH_TILES || t + 1 == t_hi) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int info = sinfo[s];
        if (info != 0) {
          const int l = info & 15;
          const int ni = nin.at(l), d = dl.at(l), off = poff.at(l);
          const int i = 16 * (info >> 8) + lr;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 16 * ((info >> 4) & 15) + M::row(lane, r);
            if (j < d && i <= ni) {
              double* p = slot + off + (i < ni ? j * ni + i : d * ni + j);
              const double v = (double)acc[s][r];
              *p = first ? v : *p + v;
            }
          }
          acc[s] = V{T(0), T(0), T(0), T(0)};
        }
      }
      first = false;
      since = 0;
    }
  }
}

// out[p] = the sum of the workgroups' slots of parameter p, in ascending order, in fp64 (zero slots: 0)
template <typename T>
__global__ void __launch_bounds__(PARAM_GRAD_BLOCK) policy_param_grad_reduce_kernel(const double* __restrict__ partial, int groups, int n_params,
                                                                                    T* __restrict__ out) {
  const int p = blockIdx.x * PARAM_GRAD_BLOCK + threadIdx.x;
  if (p >= n_params) return;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += partial[(int64_t)g * n_params + p];
  out[p] = (T)s;
}

template <typename T> static int launch_policy_param_grad_t(int64_t B, int64_t K, int32_t substeps, const excenv_policy_param_grad_t& c, hipStream_t stream) {
  const char* fn = "excenv_policy_param_grad";
  const excenv_policy_t& p = c.policy;
  static_assert(PARAM_GRAD_SLOTS * 4 >= 2 * 4 + 2 * 4 * 5 + 5, "a slot for every output tile of the widest network");
  ParamGradArgs<T> ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.nbt = (B + PARAM_GRAD_TILE - 1) / PARAM_GRAD_TILE;
  ka.tiles = policy_param_grad_tiles(B, K);
  ka.obs_krow = (int64_t)substeps * p.widths[0] * B;
  ka.groups = (int32_t)policy_param_grad_groups(B, K, c.max_groups);
  ka.n_params = (int32_t)policy_param_count(p);
  ka.n_layers = p.n_layers;
  ka.activation = p.activation;
  for (int l = 0; l <= p.n_layers; ++l) ka.widths[l] = p.widths[l];
  ka.obs = (const T*)c.obs_traj;
  ka.graw = (const T*)c.grad_raw;
  ka.partial = (double*)c.workspace;
  const dim3 block(PARAM_GRAD_BLOCK);
  if (ka.groups > 0)
    launch_dyn(policy_param_grad_kernel<T>, dim3((unsigned)ka.groups), block, policy_param_grad_lds_bytes(p, sizeof(T)), stream, ka,
               (const T*)p.params);
  if (!g_attr_failed)
    hipLaunchKernelGGL((policy_param_grad_reduce_kernel<T>), dim3((unsigned)((ka.n_params + PARAM_GRAD_BLOCK - 1) / PARAM_GRAD_BLOCK)), block, 0,
                       stream, (const double*)ka.partial, (int)ka.groups, (int)ka.n_params, (T*)c.grad_params);
  g_last_launch = policy_param_grad_name();
  return check_launch(fn);
}

int launch_policy_param_grad(int dtype, int64_t B, int64_t K, int32_t substeps, const excenv_policy_param_grad_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_policy_param_grad_t<float>(B, K, substeps, call, stream)
                             : launch_policy_param_grad_t<double>(B, K, substeps, call, stream);
}

}  // namespace excenv
