// octl_forest_prune: drop the top-level voxels that hold no point any more and collapse the empty subtrees of the
// rest, on the device, by one stable renumbering of the node table.  prune_map.h has the rules and the order of the
// steps; query.prune_np (Python) is the definition the tests compare with.  The inverse of the renumbering that
// forest_insert_incremental does when late voxels are ADDED (incremental.hip).
#include <algorithm>

#include "build_common.h"
#include "forest.h"
#include "prune_map.h"

namespace {

struct PruneLayout {
  size_t n;  // nodes (at least one)
  Carve plan;
  Carve::Part<uint32_t> occ = plan.add<uint32_t>(n), res = plan.add<uint32_t>(PRUNE_WORDS);  // (zeroed by ONE fill)
  Carve::Part<uint32_t> keep = plan.add<uint32_t>(n), new_id = plan.add<uint32_t>(n);
  Carve::Part<int32_t> node_map = plan.add<int32_t>(n);
  explicit PruneLayout(int64_t nodes) : n((size_t)(nodes > 1 ? nodes : 1)) {}
};

PruneCols prune_cols(NodeTable& t) {
  const NodePtrs p = node_ptrs(t);
  return PruneCols{p.start, p.count, p.scount, p.depth, p.voxel, p.parent, p.first_child, p.old_id, p.epoch,
                   p.corner, p.edge};
}

__global__ __launch_bounds__(256) void k_prune_mark(const int32_t* __restrict__ blk_node, int64_t n_blocks,
                                                    int64_t n_nodes, const int32_t* __restrict__ parent,
                                                    uint32_t* __restrict__ occ) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const int32_t node = blk_node[b];
  if (node < 0 || node >= n_nodes) return;  // (a damaged table marks nothing instead of writing outside occ)
  prune_mark_climb(node, parent, occ);
}

__global__ __launch_bounds__(256) void k_prune_flags(const int32_t* __restrict__ parent,
                                                     const int32_t* __restrict__ first_child,
                                                     const uint32_t* __restrict__ occ, int64_t n_nodes,
                                                     int64_t n_voxels, int mode, PruneSegs segs,
                                                     uint32_t* __restrict__ keep, uint32_t* __restrict__ res) {
  __shared__ uint32_t cnt[PRUNE_WORDS];
  for (int w = threadIdx.x; w < PRUNE_WORDS; w += 256) cnt[w] = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_nodes) {
    const bool k = prune_keep(i, mode, parent, occ);
    keep[i] = k ? 1u : 0u;
    if (k) {
      atomicAdd(&cnt[PRUNE_W_SEG + prune_seg_of(segs, i)], 1u);
      if (i < n_voxels) atomicAdd(&cnt[PRUNE_W_VOXELS], 1u);
      if (first_child[i] >= 0) atomicAdd(&cnt[occ[i] ? PRUNE_W_INTERNAL : PRUNE_W_COLLAPSED], 1u);
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < PRUNE_W_SEG + segs.n; w += 256)
    if (w != PRUNE_W_TOTAL && cnt[w]) atomicAdd(&res[w], cnt[w]);
}

__global__ __launch_bounds__(256) void k_prune_nodes(PruneCols src, PruneCols dst, const uint32_t* __restrict__ occ,
                                                     const uint32_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ new_id, int64_t n_nodes,
                                                     int64_t n_voxels, const uint64_t* __restrict__ vcode_in,
                                                     uint64_t* __restrict__ vcode_out, int32_t* __restrict__ node_map) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  prune_write_node(i, src, dst, occ, keep, new_id, n_voxels, vcode_in, vcode_out, node_map);
}

__global__ __launch_bounds__(256) void k_prune_blocks(int32_t* __restrict__ blk_node, int64_t n_blocks,
                                                      int64_t n_nodes, const int32_t* __restrict__ node_map) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const int32_t node = blk_node[b];
  if (node >= 0 && node < n_nodes) blk_node[b] = node_map[node];
}

}  // namespace

extern "C" int octl_forest_prune(octl_forest* f, int64_t cap_nodes, int32_t* node_map, int32_t* old_node,
                                 octl_prune_info* info) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (info) *info = octl_prune_info{0, 0, 0, 0, 0, 0};
  if (!f->built) return OCTL_OK;  // (no tables: never built, or reset by octl_forest_transform_poses - no launch)
  if (f->store_dirty)
    return octl_set_error(ctx, OCTL_E_STATE,
                          "prune: points were added since the forest was built (bring it up to date first)");
  NodeTable& cur = f->nodes[f->cur];
  const int64_t N = cur.n, V = f->n_voxels, nb = f->n_blocks;
  if ((node_map || old_node) && cap_nodes < N)
    return octl_set_error(ctx, OCTL_E_INVALID, "prune: room for %lld node ids, the map has %lld nodes",
                          (long long)cap_nodes, (long long)N);
  if (info) {
    info->nodes_before = info->nodes_after = N;
    info->voxels_before = info->voxels_after = V;
    info->internal_after = f->n_internal;
  }
  if (N == 0) return OCTL_OK;
  // the level ranges as the kernel counts by them: they tile [0, N) in the order the builds appended them
  PruneSegs segs;
  std::memset(&segs, 0, sizeof segs);
  {
    if (f->level_segs.empty() || f->level_segs.size() > PRUNE_MAX_SEGS)
      return octl_set_error(ctx, OCTL_E_STATE, "prune: %zu level ranges (1 .. %d can be rewritten)",
                            f->level_segs.size(), PRUNE_MAX_SEGS);
    int64_t at = 0;
    for (const auto& sg : f->level_segs) {
      if (sg.a != at || sg.b < sg.a)
        return octl_set_error(ctx, OCTL_E_STATE, "prune: the level ranges do not tile the node table");
      at = sg.b;
      segs.end[segs.n++] = sg.b;
    }
    if (at != N || f->level_segs[0].b != V)
      return octl_set_error(ctx, OCTL_E_STATE, "prune: the level ranges do not tile the node table");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // ---- every buffer before anything the forest reads is changed: a failed allocation leaves it as it was ---------
  const PruneLayout lay(N);
  OCTL_TRY(devbuf_reserve(ctx, f->entries, lay.plan.total));
  OCTL_TRY(octl_exclusive_scan_reserve(ctx, N));
  NodeTable& nxt = f->nodes[f->cur ^ 1];
  OCTL_TRY(nodes_reserve(ctx, nxt, N));
  OCTL_TRY(devbuf_reserve(ctx, f->vcode_dev[1], (size_t)std::max<int64_t>(V, 1) * 8));
  // the packed keys on the device: what the forest reads its voxels from afterwards.  (An upload of the host's copy is
  // not waited for here: the call's one wait comes before anything can change that copy.)
  OCTL_TRY(forest_sync_vcodes(f, false));
  uint32_t* occ = Carve::at(f->entries, lay.occ);
  uint32_t* res = Carve::at(f->entries, lay.res);
  uint32_t* keep = Carve::at(f->entries, lay.keep);
  uint32_t* new_id = Carve::at(f->entries, lay.new_id);
  int32_t* map_d = Carve::at(f->entries, lay.node_map);
  const PruneCols src = prune_cols(cur), dst = prune_cols(nxt);
  uint32_t got[PRUNE_WORDS];
  {
    KTimer t(ctx, "prune_mark");
    HIP_TRY(ctx, hipMemsetAsync(occ, 0, lay.keep.off - lay.occ.off, st));  // occ and the counters
    if (nb > 0) {
      OCTL_LAUNCH(k_prune_mark, dim3(grid_for(nb)), dim3(256), 0, st, (const int32_t*)f->blk_node.as<int32_t>(), nb, N,
                  (const int32_t*)src.parent, occ);
      HIP_TRY(ctx, hipGetLastError());
    }
    OCTL_LAUNCH(k_prune_flags, dim3(grid_for(N)), dim3(256), 0, st, (const int32_t*)src.parent,
                (const int32_t*)src.first_child, (const uint32_t*)occ, N, V, f->mode, segs, keep, res);
    HIP_TRY(ctx, hipGetLastError());
    OCTL_TRY(octl_exclusive_scan_u32(ctx, keep, new_id, N, res + PRUNE_W_TOTAL));
  }
  // the one host wait: the counts through the context's mirror
  OCTL_TRY(octl_readback(ctx, res, PRUNE_W_SEG + segs.n, got));
  int64_t seg_a[PRUNE_MAX_SEGS], seg_b[PRUNE_MAX_SEGS];
  const int64_t n_new = prune_rewrite_segs(segs.n, got + PRUNE_W_SEG, seg_a, seg_b);
  const int64_t v_new = got[PRUNE_W_VOXELS], collapsed = got[PRUNE_W_COLLAPSED];
  if (n_new != (int64_t)got[PRUNE_W_TOTAL] || n_new > N || v_new > V || seg_b[0] != v_new)
    return octl_set_error(ctx, OCTL_E_STATE, "prune: the counts of the kept nodes disagree (%lld by level, %u scanned)",
                          (long long)n_new, got[PRUNE_W_TOTAL]);
  const bool identity = n_new == N && collapsed == 0;
  if (!identity) {
    KTimer t(ctx, "prune_nodes");
    OCTL_LAUNCH(k_prune_nodes, dim3(grid_for(N)), dim3(256), 0, st, src, dst, (const uint32_t*)occ,
                (const uint32_t*)keep, (const uint32_t*)new_id, N, V,
                (const uint64_t*)f->vcode_dev[0].as<uint64_t>(), f->vcode_dev[1].as<uint64_t>(), map_d);
    HIP_TRY(ctx, hipGetLastError());
    if (nb > 0) {  // last: up to here nothing the forest reads has been written
      OCTL_LAUNCH(k_prune_blocks, dim3(grid_for(nb)), dim3(256), 0, st, f->blk_node.as<int32_t>(), nb, N,
                  (const int32_t*)map_d);
      HIP_TRY(ctx, hipGetLastError());
    }
    // ---- commit ---------------------------------------------------------------------------------------------------
    f->cur ^= 1;
    std::swap(f->vcode_dev[0], f->vcode_dev[1]);
    nxt.n = n_new;
    f->n_voxels = v_new;
    f->n_internal = got[PRUNE_W_INTERNAL];
    f->vkeys_stale = true;  // (forest_sync_vkeys downloads the codes)
    std::vector<octl_forest::LevelSeg> kept_segs;
    int32_t deepest = 0;
    for (int s = 0; s < segs.n; ++s) {
      if (s > 0 && seg_b[s] == seg_a[s]) continue;  // (the roots' range stays, empty or not)
      kept_segs.push_back({seg_a[s], seg_b[s], f->level_segs[(size_t)s].depth});
      if (seg_b[s] > seg_a[s]) deepest = std::max(deepest, (int32_t)f->level_segs[(size_t)s].depth);
    }
    f->level_segs.swap(kept_segs);
    f->max_depth_reached = deepest;
    f->fast_order_valid = false;
    f->split_stats_valid = false;
    forest_contents_changed(f);
  }
  if (info) {
    info->nodes_after = n_new;
    info->voxels_after = v_new;
    info->internal_after = f->n_internal;
    info->collapsed = collapsed;
  }
  if (identity) {
    for (int64_t i = 0; i < N; ++i) {
      if (node_map) node_map[i] = (int32_t)i;
      if (old_node) old_node[i] = (int32_t)i;
    }
    return OCTL_OK;
  }
  if (node_map || (old_node && n_new > 0)) {  // (asked for: a second wait behind the two passes)
    if (node_map) HIP_TRY(ctx, hipMemcpyAsync(node_map, map_d, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    if (old_node && n_new > 0)
      HIP_TRY(ctx, hipMemcpyAsync(old_node, nxt.old_id.p, (size_t)n_new * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return OCTL_OK;
}
