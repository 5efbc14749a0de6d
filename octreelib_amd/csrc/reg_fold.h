// What the kernels of the three registration systems share beside the arithmetic of a term: the transform of a query,
// the chunk size of the first half of the reduction and k_reg_fold, the second half, which folds the rows of per-chunk
// sums into the 28 + 2 numbers of a call.  Shared by register.hip (k_reg_partial), register_points.hip (k_regp_partial)
// and register_nearest_plane.hip (k_regn_partial): one tree, a function of n alone (register.hip has the count of
// additions).
#pragma once
#include "sums28.h"

__device__ __forceinline__ void reg_transform(const double* __restrict__ T, double qx, double qy, double qz,
                                              double p[3]) {
  // (separate products and sums: the library is built with -ffp-contract=off, and the host forms the same bits)
  p[0] = ((T[0] * qx + T[1] * qy) + T[2] * qz) + T[3];
  p[1] = ((T[4] * qx + T[5] * qy) + T[6] * qz) + T[7];
  p[2] = ((T[8] * qx + T[9] * qy) + T[10] * qz) + T[11];
}

namespace {

constexpr int RS_CHUNK = 4096;  // consecutive queries per workgroup of the first half, one scratch row each

__global__ __launch_bounds__(256) void k_reg_fold(const double* __restrict__ rows, int64_t n_rows,
                                                  double* __restrict__ sys, int64_t* __restrict__ counts) {
  __shared__ double lds[4][RS_SUMS];
  __shared__ long long ldc[4][2];
  RegAcc a;
  reg_zero(a);
  for (int64_t r = threadIdx.x; r < n_rows; r += 256) {
    const double* in = rows + r * RS_ROW;
#pragma unroll
    for (int k = 0; k < RS_SUMS; ++k) a.s[k] += in[k];
    a.used += reinterpret_cast<const long long*>(in)[RS_SUMS];
    a.located += reinterpret_cast<const long long*>(in)[RS_SUMS + 1];
  }
  reg_block_reduce(a, lds, ldc);
  if (threadIdx.x < RS_SUMS) sys[threadIdx.x] = a.s[0];
  if (threadIdx.x == 0) {
    counts[0] = a.used;
    counts[1] = a.located;
  }
}

}  // namespace
