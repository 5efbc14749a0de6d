// The 28 sums + 2 counts of a 6x6 point-to-plane system and their reduction over a workgroup of 256: shared by
// register.hip (k_reg_partial), register_points.hip (k_regp_partial), register_nearest_plane.hip (k_regn_partial),
// reg_fold.h (k_reg_fold) and adjust.hip (k_adj_partial / k_adj_fold) - one fixed tree.
#pragma once
#include "common.h"

namespace {

constexpr int RS_SUMS = 28;   // 21 of H, 6 of g, the cost
constexpr int RS_ROW = 32;    // doubles per scratch row: the sums, the two counts (int64 bits), padding to 256 bytes

struct RegAcc {
  double s[RS_SUMS];
  long long used, located;
};

__device__ __forceinline__ void reg_zero(RegAcc& a) {
#pragma unroll
  for (int k = 0; k < RS_SUMS; ++k) a.s[k] = 0.0;
  a.used = a.located = 0;
}

// wave butterfly, then the workgroup's four waves in wave order; threads [0, 28) leave with the total of sum `tid` in
// a.s[0], thread 0 with the two counts
__device__ __forceinline__ void reg_block_reduce(RegAcc& a, double (*lds)[RS_SUMS], long long (*ldc)[2]) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < RS_SUMS; ++k) a.s[k] += __shfl_xor(a.s[k], m);
    a.used += __shfl_xor(a.used, m);
    a.located += __shfl_xor(a.located, m);
  }
  const int tid = threadIdx.x, wave = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < RS_SUMS; ++k) lds[wave][k] = a.s[k];
    ldc[wave][0] = a.used;
    ldc[wave][1] = a.located;
  }
  __syncthreads();
  if (tid < RS_SUMS) a.s[0] = ((lds[0][tid] + lds[1][tid]) + lds[2][tid]) + lds[3][tid];
  if (tid == 0) {
    a.used = ldc[0][0] + ldc[1][0] + ldc[2][0] + ldc[3][0];
    a.located = ldc[0][1] + ldc[1][1] + ldc[2][1] + ldc[3][1];
  }
}

// what reg_block_reduce left, into the scratch row of this workgroup (the epilogue of the three *_partial kernels)
__device__ __forceinline__ void reg_write_row(const RegAcc& a, double* __restrict__ rows) {
  double* out = rows + (int64_t)blockIdx.x * RS_ROW;
  if (threadIdx.x < RS_SUMS) out[threadIdx.x] = a.s[0];
  if (threadIdx.x == 0) {
    reinterpret_cast<long long*>(out)[RS_SUMS] = a.used;
    reinterpret_cast<long long*>(out)[RS_SUMS + 1] = a.located;
  }
}

}  // namespace
