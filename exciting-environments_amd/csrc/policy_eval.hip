// The network of excenv_sim_policy on stored observation rows (excenv_policy_eval, include/excenv.h):
//   out[r][q][b] = x^L[q] of mlp(obs[r * row_stride][.][b])
// the forward half beside policy_param_grad.hip, product 1 of its kernel carried through every layer. It needs no model: two
// instantiations, one per element type. An f32 MFMA (v_mfma_f32_16x16x4_f32) is bit for bit a k-ordered fmaf chain, so with C
// starting at the bias and k running over the inputs in ascending order a result is the bits sim_policy_kernel's own chain gives;
// POLICY_EVAL_F64_MMA (policy.hpp) says whether the fp64 instantiation multiplies with v_mfma_f64_16x16x4_f64 or by per-lane fma chains.
//   A sample tile is 64 consecutive environments of one evaluated row, read 64 wide from the lane-major array (tail lanes load zeros
// and store nothing). It lives in dynamic LDS as rows [unit][sample] of PARAM_GRAD_LDS_STRIDE elements (policy.hpp): x^0 twice, so
// the next tile is staged while this one is read, and two buffers the hidden layers alternate between. Per layer A = W_l from
// global memory, B = x^{l-1} from LDS, C starts at b_l. Wave w owns the samples 16 w .. 16 w + 15 through every layer and reads only
// the columns it wrote: behind the one barrier that follows the staging of x^0 no wave depends on another. The output layer is the
// same product with at most two rows of its 16-row tile live; every wave stores its 16 consecutive environments of each output row.
// Dimensions that are no multiple of 16 or 4 are filled by a select on the operand behind a clamped index: nothing is read out of
// bounds. A filled step is fma(-0, +0, c) = c for every c, a zero of either sign included.
// Which tiles a workgroup owns is a function of (B, R) alone. No atomics, no inline assembly, no scratch, no static LDS.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels_policy.hpp"

namespace excenv {

template <typename T> struct PolicyEvalArgs {
  int64_t B, nbt, tiles;  // nbt = ceil(B / 64) tiles per evaluated row
  int64_t obs_rrow;       // elements between the observation rows of two evaluated rows: row_stride * OW * B
  int32_t groups;
  int32_t n_layers, activation;
  int32_t widths[EXCENV_POLICY_MAX_LAYERS + 1];
  const T* obs;  // [(R - 1) * row_stride + 1 or more][OW][B]
  T* out;        // [R][A][B]
};

// lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]; result register r of lane l is row(l, r), column l & 15
template <typename T> struct EvalMma;
template <> struct EvalMma<float> {
  typedef float V __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ V mma(float a, float b, V c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};
template <> struct EvalMma<double> {
  typedef double V __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ V mma(double a, double b, V c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }  // (not the f32 map)
};

extern __shared__ __attribute__((aligned(16))) unsigned char policy_eval_lds[];

// one value per layer l = 1 .. 4, picked by compares
struct EvalTab4 {
  int a, b, c, d;
  __device__ __forceinline__ int at(int l) const { return l == 1 ? a : l == 2 ? b : l == 3 ? c : d; }
};
static_assert(EXCENV_POLICY_MAX_LAYERS == 4, "EvalTab4");

// The lanes of a wave exchange a layer through LDS: the stores of x^l come before the loads of the next layer, for the compiler too
static __device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ void __launch_bounds__(PARAM_GRAD_BLOCK) policy_eval_kernel(const PolicyEvalArgs<T> ka, const T* __restrict__ params) {
  using M = EvalMma<T>;
  using V = typename M::V;
  constexpr bool MMA = sizeof(T) == 4 || POLICY_EVAL_F64_MMA;
  constexpr int LD = PARAM_GRAD_LDS_STRIDE, TILE = PARAM_GRAD_TILE;
  constexpr int NPRE = (EXCENV_POLICY_MAX_INPUT + 3) / 4;  // staged rows per wave
  T* const lds = reinterpret_cast<T*>(policy_eval_lds);
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = ka.n_layers, activation = ka.activation;

  // per layer l, in scalar registers (no arrays: nothing here may be indexed at run time): inputs, outputs, where W_l starts
  const int w0 = ka.widths[0], w1 = ka.widths[1], w2 = L >= 2 ? ka.widths[2] : 1, w3 = L >= 3 ? ka.widths[3] : 1, w4 = L >= 4 ? ka.widths[4] : 1;
  const EvalTab4 nin{w0, L >= 2 ? w1 : 1, L >= 3 ? w2 : 1, L >= 4 ? w3 : 1}, dl{w1, w2, w3, w4};
  const int sz1 = dl.a * (nin.a + 1), sz2 = L >= 2 ? dl.b * (nin.b + 1) : 0, sz3 = L >= 3 ? dl.c * (nin.c + 1) : 0;
  const EvalTab4 poff{0, sz1, sz1 + sz2, sz1 + sz2 + sz3};
  const int OW = w0, A = dl.at(L);
  // the LDS rows (policy_eval_lds_rows): x^0 of even / odd tiles at 0 / OW, x^1 and x^3 at 2 OW, x^2 behind the wider of the two
  const int h1 = L >= 2 ? w1 : 0, h3 = L >= 4 ? w3 : 0;
  const int hrow_odd = 2 * OW, hrow_even = 2 * OW + (h1 > h3 ? h1 : h3);

  const int64_t g = blockIdx.x;
  const int64_t tq = ka.tiles / ka.groups, tr = ka.tiles % ka.groups;
  const int64_t t_lo = g * tq + (g < tr ? g : tr), t_hi = (g + 1) * tq + (g + 1 < tr ? g + 1 : tr);

  // the rows of tile t this wave stages: row wave + 4 r of x^0
  auto load_tile = [&](int64_t t, T (&pre)[NPRE]) __attribute__((always_inline)) {
    const int64_t r = t / ka.nbt;
    const int64_t b = (t - r * ka.nbt) * TILE + lane;
    const bool live = b < ka.B;
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int row = wave + 4 * i;
      pre[i] = T(0);
      if (row < OW && live) pre[i] = ka.obs[r * ka.obs_rrow + (int64_t)row * ka.B + b];
    }
  };

  const int scol = 16 * wave + lr;  // the sample column of this lane
  int buf = 0;
  T pre[NPRE];
  load_tile(t_lo, pre);
  for (int64_t t = t_lo; t < t_hi; ++t) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int row = wave + 4 * i;
      if (row < OW) lds[(buf * OW + row) * LD + lane] = pre[i];
    }
    // the one barrier of a tile. A wave that stages tile t + 1 into the other x^0 buffer has passed this barrier, so every wave has
    // left tile t - 1, the last reader of that buffer
    __syncthreads();
    if (t + 1 < t_hi) load_tile(t + 1, pre);
    const int64_t r = t / ka.nbt;
    const int64_t b = (t - r * ka.nbt) * TILE + scol;
    const bool live = b < ka.B;

    for (int l = 1; l <= L; ++l) {
      const int ni = nin.at(l), d = dl.at(l), off = poff.at(l);
      const bool last = l == L;
      const T* xin = lds + (l == 1 ? buf * OW : ((l - 1) & 1) ? hrow_odd : hrow_even) * LD + scol;
      T* xout = lds + ((l & 1) ? hrow_odd : hrow_even) * LD + scol;
      T* orow = ka.out + r * A * ka.B + b;
      const T* bias = params + off + d * ni;
      auto emit = [&](int j, T y) __attribute__((always_inline)) {
        if (last) {
          if (live) orow[(int64_t)j * ka.B] = y;
        } else {
          xout[j * LD] = policy_act(y, activation);
        }
      };
      if constexpr (MMA) {
        for (int j0 = 0; j0 < d; j0 += 16) {
          V c;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = j0 + M::row(lane, q);
            c[q] = bias[j < d ? j : d - 1];
          }
          const bool jok = j0 + lr < d;
          const T* w = params + off + (jok ? j0 + lr : d - 1) * ni;
          for (int i0 = 0; i0 < ni; i0 += 4) {
            const int i = i0 + lq;
            const bool iok = i < ni;
            const int ic = iok ? i : ni - 1;
            const T a = w[ic], x = xin[ic * LD];
            c = M::mma((iok && jok) ? a : T(-0.0), iok ? x : T(0), c);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = j0 + M::row(lane, q);
            if (j < d) emit(j, c[q]);
          }
        }
      } else {
        // the chain itself: the four lanes of a sample share its units, j = lq, lq + 4, ..
        for (int j = lq; j < d; j += 4) {
          const T* w = params + off + j * ni;
          T acc = bias[j];
          for (int i = 0; i < ni; ++i) acc = xfma(w[i], xin[i * LD], acc);
          emit(j, acc);
        }
      }
      wave_lds_order();
    }
    buf ^= 1;
  }
}

template <typename T> static int launch_policy_eval_t(int64_t B, int64_t R, int64_t row_stride, const excenv_policy_eval_t& c, hipStream_t stream) {
  const excenv_policy_t& p = c.policy;
  PolicyEvalArgs<T> ka;
  std::memset(&ka, 0, sizeof(ka));
  ka.B = B;
  ka.nbt = (B + PARAM_GRAD_TILE - 1) / PARAM_GRAD_TILE;
  ka.tiles = policy_eval_tiles(B, R);
  ka.obs_rrow = row_stride * p.widths[0] * B;
  ka.groups = (int32_t)policy_eval_groups(B, R);
  ka.n_layers = p.n_layers;
  ka.activation = p.activation;
  for (int l = 0; l <= p.n_layers; ++l) ka.widths[l] = p.widths[l];
  ka.obs = (const T*)c.obs_traj;
  ka.out = (T*)c.out;
  launch_dyn(policy_eval_kernel<T>, dim3((unsigned)ka.groups), dim3(PARAM_GRAD_BLOCK), policy_eval_lds_bytes(p, sizeof(T)), stream, ka,
             (const T*)p.params);
  g_last_launch = policy_eval_name();
  return check_launch("excenv_policy_eval");
}

int launch_policy_eval(int dtype, int64_t B, int64_t R, int64_t row_stride, const excenv_policy_eval_t& call, hipStream_t stream) {
  return dtype == EXCENV_F32 ? launch_policy_eval_t<float>(B, R, row_stride, call, stream)
                             : launch_policy_eval_t<double>(B, R, row_stride, call, stream);
}

}  // namespace excenv
