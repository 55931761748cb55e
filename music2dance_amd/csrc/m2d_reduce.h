// The library's one fixed-order fp64 block sum (pointwise.hip, cond.hip, distrib.hip, spectral.hip). Every result
// that is "the same bits on every run" rests on this order: thread t's value lands in sh[t], then
// sh[t] += sh[t + s] for s = N/2, N/4, ..., 1 - a binary tree whose shape depends on N alone.
//
// Contract: the workgroup has exactly N threads (a power of two) and all of them call; sh holds N doubles and no thread
// still reads or writes it on entry - which is true after a previous m2d_block_sum on the same array has returned (the
// trailing barrier), and after any barrier that follows the caller's own last use of sh. The first barrier inside
// orders every earlier LDS write of the caller before the tree. Every thread gets the sum.
//
// Separate on purpose: the two-value trees inside m2d_bn_reduce_kernel (bn.hip) and m2d_rowsums_reduce_kernel
// (gemm_engine.hip) - training hot path, their data already sits in LDS in another layout - the stage kernels of
// m2d_rowsums_reduce, and every __shfl_xor wave reduction (gemm_engine.hip, conv1d_thin.hip, tcn.hip, the
// cross-entropy row of pointwise.hip).
#pragma once
#include <hip/hip_runtime.h>

template <int N>
__device__ __forceinline__ double m2d_block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
