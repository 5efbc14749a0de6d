// The shifted-moment reduction of one (leaf, pose) block and the (node, slot) grouping of the selected blocks: shared by
// leaf_stats.hip (octl_forest_leaf_stats, octl_forest_pooled_leaf_stats) and adjust.hip (the block moments table of
// octl_forest_adjustment_system), so that a block's sums are the same bits wherever they are formed.
#pragma once
#include "common.h"

namespace {

constexpr int LS_CHUNK = 64 * 64;  // L: points per chunk of a large block

struct Sums {
  double s[9];  // sum dx, dy, dz; sum dx dx, dx dy, dx dz, dy dy, dy dz, dz dz
};

// P_c: the moments of points [first, first + cnt) relative to p0, reduced over the wave; every lane returns them
__device__ __forceinline__ Sums chunk_sums(const double* __restrict__ xyz, int64_t first, int cnt, double p0x,
                                           double p0y, double p0z, int lane) {
  Sums a;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.s[k] = 0.0;
  for (int j = lane; j < cnt; j += 64) {
    const double* p = xyz + 3 * (first + j);
    const double dx = p[0] - p0x, dy = p[1] - p0y, dz = p[2] - p0z;
    a.s[0] += dx;
    a.s[1] += dy;
    a.s[2] += dz;
    a.s[3] = fma(dx, dx, a.s[3]);
    a.s[4] = fma(dx, dy, a.s[4]);
    a.s[5] = fma(dx, dz, a.s[5]);
    a.s[6] = fma(dy, dy, a.s[6]);
    a.s[7] = fma(dy, dz, a.s[7]);
    a.s[8] = fma(dz, dz, a.s[8]);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int k = 0; k < 9; ++k) a.s[k] += __shfl_xor(a.s[k], m);
  return a;
}

__device__ __forceinline__ void fold(Sums& acc, const Sums& p) {
#pragma unroll
  for (int k = 0; k < 9; ++k) acc.s[k] = acc.s[k] + p.s[k];
}

__device__ __forceinline__ void finish(const Sums& S, int64_t n, double p0x, double p0y, double p0z, double* mean,
                                       double* cov) {
  const double dn = (double)n;
  const double mx = S.s[0] / dn, my = S.s[1] / dn, mz = S.s[2] / dn;
  mean[0] = p0x + mx;
  mean[1] = p0y + my;
  mean[2] = p0z + mz;
  cov[0] = fma(-mx, mx, S.s[3] / dn);
  cov[1] = fma(-mx, my, S.s[4] / dn);
  cov[2] = fma(-mx, mz, S.s[5] / dn);
  cov[3] = fma(-my, my, S.s[6] / dn);
  cov[4] = fma(-my, mz, S.s[7] / dn);
  cov[5] = fma(-mz, mz, S.s[8] / dn);
}

__global__ __launch_bounds__(256) void k_pool_keys(const int32_t* __restrict__ blk_node,
                                                   const int32_t* __restrict__ blk_slot, int64_t nb,
                                                   const uint8_t* __restrict__ sel, int n_sel, int sbits, int kbits,
                                                   uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const int32_t s = blk_slot[b];
  const bool on = !sel || (s >= 0 && s < n_sel && sel[s] != 0);
  // (an unselected block sorts behind every selected one: bit kbits is above any (node, slot) key)
  key[b] = on ? (((uint64_t)(uint32_t)blk_node[b] << sbits) | (uint64_t)(uint32_t)s) : (1ull << kbits);
  val[b] = (uint32_t)b;
}

__global__ __launch_bounds__(256) void k_pool_heads(const uint64_t* __restrict__ key, int64_t nb, int sbits, int kbits,
                                                    uint32_t* __restrict__ heads) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const uint64_t k = key[i];
  heads[i] = ((k >> kbits) == 0 && (i == 0 || (key[i - 1] >> sbits) != (k >> sbits))) ? 1u : 0u;
}

}  // namespace
