// The shifted-moment reduction of one (leaf, pose) block - shared by leaf_stats.hip (octl_forest_leaf_stats,
// octl_forest_pooled_leaf_stats) and adjust.hip (the block moments table of octl_forest_adjustment_system), so that a
// block's sums are the same bits wherever they are formed - and the (node, slot) grouping of the selected blocks, kernels
// and host driver (block_groups), that the pooled planes, the adjustment tables and the neighbour index start from.
#pragma once
#include <algorithm>

#include "common.h"
#include "forest.h"

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

__host__ __device__ __forceinline__ void finish(const Sums& S, int64_t n, double p0x, double p0y, double p0z,
                                                double* mean, double* cov) {
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

// The selected blocks of the forest grouped by leaf: (node << sbits | slot, block id) pairs sorted by key, a block of
// an unselected pose behind every selected one (bit kbits), and with `rows` the exclusive scan of the flags "first
// selected block of its node" - the row of a leaf in ascending node id at its head, one more at the positions behind.
// `plan` starts with the grouping's parts of f->grp_scratch; the caller adds what it needs besides, then prepare()
// reserves the buffer, fills in the pointers and sends the selection, and block_groups launches.
struct BlockGroups {
  size_t nb, n_poses;
  bool rows;
  int sbits = std::max(1, bits_for(n_poses)), nbits, kbits = sbits + nbits;  // bits of a slot, a node id, a key
  Carve plan;
  Carve::Part<uint64_t> key_part[2] = {plan.add<uint64_t>(nb), plan.add<uint64_t>(nb)};
  Carve::Part<uint32_t> val_part[2] = {plan.add<uint32_t>(nb), plan.add<uint32_t>(nb)},
                        heads_part = plan.add<uint32_t>(rows ? nb + 8 : 0);  // (+8: the scan's tail)
  Carve::Part<uint8_t> sel_part = plan.add<uint8_t>(n_poses);
  uint64_t* keys[2] = {nullptr, nullptr};  // (set by prepare) [0] the sorted keys, [1] the other buffer (free)
  uint32_t* vals[2] = {nullptr, nullptr};  // ... and the block ids
  uint32_t* heads = nullptr;               // [n_blocks] the scanned head flags (rows only)
  uint8_t* sel_d = nullptr;                // the selection on the device (nullptr: every pose)
  BlockGroups(const octl_forest* f, bool want_rows)
      : nb((size_t)f->n_blocks), n_poses(std::max<size_t>(f->pose_off.size() - 1, 1)), rows(want_rows),
        nbits(std::max(1, bits_for((uint64_t)f->nodes[f->cur].n))) {}
  int prepare(octl_forest* f, const std::vector<uint8_t>& sel) {
    DevBuf& b = f->grp_scratch;
    OCTL_TRY(devbuf_reserve(f->ctx, b, plan.total));
    for (int i = 0; i < 2; ++i) keys[i] = Carve::at(b, key_part[i]), vals[i] = Carve::at(b, val_part[i]);
    heads = rows ? Carve::at(b, heads_part) : nullptr;
    sel_d = sel.empty() ? nullptr : Carve::at(b, sel_part);
    if (sel_d) HIP_TRY(f->ctx, hipMemcpyAsync(sel_d, sel.data(), sel.size(), hipMemcpyHostToDevice, f->ctx->stream));
    return OCTL_OK;
  }
};

// f->n_blocks > 0, g.prepare has run.  n_sel: entries of the selection (0: every pose); total_d: the device word of the
// caller's that receives the number of rows (rows only; the caller reads it back).  The caller times the launches under
// its own KTimer name (pool_group, adj_group, nn_group) with whatever else of its own belongs to that region.
int block_groups(octl_forest* f, int n_sel, uint32_t* total_d, BlockGroups& g) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const int64_t nb = f->n_blocks;
  OCTL_LAUNCH(k_pool_keys, dim3(grid_for(nb)), dim3(256), 0, st, (const int32_t*)f->blk_node.as<int32_t>(),
              (const int32_t*)f->blk_slot.as<int32_t>(), nb, (const uint8_t*)g.sel_d, n_sel, g.sbits, g.kbits, g.keys[0],
              g.vals[0]);
  HIP_TRY(ctx, hipGetLastError());
  int res = 0;
  OCTL_TRY(octl_radix_sort_u64_u32(ctx, g.keys, g.vals, nb, g.kbits + 1, f->pl_hist, &res));
  if (res) std::swap(g.keys[0], g.keys[1]), std::swap(g.vals[0], g.vals[1]);
  if (g.rows) {
    OCTL_LAUNCH(k_pool_heads, dim3(grid_for(nb)), dim3(256), 0, st, (const uint64_t*)g.keys[0], nb, g.sbits, g.kbits,
                g.heads);
    HIP_TRY(ctx, hipGetLastError());
    OCTL_TRY(octl_exclusive_scan_u32(ctx, g.heads, g.heads, nb, total_d));
  }
  return OCTL_OK;
}

}  // namespace
