// The deterministic batch sum behind excenv_param_grad_sum: out[j] = sum over the batch of the j-th per-environment gradient array
// (what excenv_sim_ahead_vjp_params wrote). Two launches, no atomics: the order of every addition is a function of B alone, so the
// same batch gives the same bits on every run, whatever form of the reverse kernel produced the per-environment values.
//   stage one: param_sum_groups(B) workgroups (vjp.hpp), each over one fixed contiguous slice of [B]; a lane adds every 256th element of
//              the slice in fp64 (coalesced), the wave reduces by shuffles, the four waves through LDS; one fp64 partial per workgroup
//              and leaf goes to the caller's workspace
//   stage two: one workgroup per leaf adds the partials the same way and stores the working dtype
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vjp.hpp"

namespace excenv {

struct ParamSumPtrs {
  const void* p[EXCENV_MAX_STATIC];
};

// the sum of v over the workgroup's 256 lanes, in lane 0 (fixed tree: shuffles within a wave, then waves 0..3 in order)
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  return s;
}

template <typename T>
__global__ void __launch_bounds__(PSUM_BLOCK) param_sum_stage1(ParamSumPtrs in, int64_t B, int64_t slice, double* __restrict__ partial) {
  __shared__ double lds[PSUM_BLOCK / 64];
  const T* x = (const T*)in.p[blockIdx.y];
  const int64_t lo = (int64_t)blockIdx.x * slice;
  const int64_t hi = (lo + slice < B) ? lo + slice : B;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += PSUM_BLOCK) acc += (double)x[i];
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <typename T>
__global__ void __launch_bounds__(PSUM_BLOCK) param_sum_stage2(const double* __restrict__ partial, int groups, T* __restrict__ out) {
  static_assert(PSUM_GROUPS <= PSUM_BLOCK, "one partial per lane");
  __shared__ double lds[PSUM_BLOCK / 64];
  const double v = ((int)threadIdx.x < groups) ? partial[(int64_t)blockIdx.x * groups + threadIdx.x] : 0.0;
  const double s = block_sum(v, lds);
  if (threadIdx.x == 0) out[blockIdx.x] = (T)s;
}

int launch_param_sum(int dtype, int64_t B, int n, const void* const* per_env, void* out, void* workspace, hipStream_t stream) {
  ParamSumPtrs in{};
  for (int j = 0; j < n; ++j) in.p[j] = per_env[j];
  const int groups = param_sum_groups(B);
  const int64_t slice = (B + groups - 1) / groups;
  const dim3 grid1((unsigned)groups, (unsigned)n), block(PSUM_BLOCK);
  double* partial = (double*)workspace;
  if (dtype == EXCENV_F32) {
    hipLaunchKernelGGL((param_sum_stage1<float>), grid1, block, 0, stream, in, B, slice, partial);
    hipLaunchKernelGGL((param_sum_stage2<float>), dim3((unsigned)n), block, 0, stream, (const double*)partial, groups, (float*)out);
  } else {
    hipLaunchKernelGGL((param_sum_stage1<double>), grid1, block, 0, stream, in, B, slice, partial);
    hipLaunchKernelGGL((param_sum_stage2<double>), dim3((unsigned)n), block, 0, stream, (const double*)partial, groups, (double*)out);
  }
  return hipGetLastError() == hipSuccess ? EXCENV_OK : EXCENV_EHIP;
}

}  // namespace excenv
