// extern "C" surface of the forest (Grid / OctreeManager / Octree state) and of the stand-alone
// RANSAC operator: lifecycle, build / scheme / contents, queries, RANSAC and debug entries.  The point
// store's entries are in store.hip, apply_mask's in mask.hip.  See include/octreelib_hip.h for the
// reference interfaces each entry point replaces.
#include <unordered_map>

#include "forest.h"

namespace {

// counters of one pose (octree.py:144-175, grid.py:343-362) without fetching the block table:
// out[0] = points, out[1] = non-empty leaves of the slot
__global__ __launch_bounds__(256) void k_slot_counts(const int32_t* __restrict__ blk_slot,
                                                     const int32_t* __restrict__ blk_size, int64_t nb,
                                                     int32_t slot, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long part[2][4];
  unsigned long long pts = 0, lv = 0;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (int64_t)gridDim.x * blockDim.x) {
    if (blk_slot[b] == slot) {
      pts += (unsigned long long)blk_size[b];
      lv += 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    pts += __shfl_xor(pts, off);
    lv += __shfl_xor(lv, off);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = pts;
    part[1][threadIdx.x >> 6] = lv;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned long long t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
    if (t) atomicAdd(&out[threadIdx.x], t);
  }
}

// internal scheme nodes per top-level voxel (n_nodes of a pose = sum over its voxels of 1 + 8 * internal)
__global__ __launch_bounds__(256) void k_internal_per_voxel(const int32_t* __restrict__ first_child,
                                                            const int32_t* __restrict__ voxel, int64_t n,
                                                            int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && first_child[i] >= 0) atomicAdd(&out[voxel[i]], 1);
}

// voxels in which a pose slot has at least one block
__global__ __launch_bounds__(256) void k_slot_voxel_flags(const int32_t* __restrict__ blk_node,
                                                          const int32_t* __restrict__ blk_slot,
                                                          int64_t nb, int32_t slot,
                                                          const int32_t* __restrict__ node_voxel,
                                                          uint32_t* __restrict__ flags) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nb && blk_slot[b] == slot) flags[node_voxel[blk_node[b]]] = 1u;
}

__global__ __launch_bounds__(256) void k_flag_indices(const uint32_t* __restrict__ flags,
                                                      const uint32_t* __restrict__ scanned, int64_t n,
                                                      int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flags[i]) out[scanned[i]] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_widen_u32_i64(const uint32_t* __restrict__ in, int64_t n,
                                                       int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int64_t)in[i];
}


// octl_forest_gather_blocks: sizes of the selected blocks, then one wavefront per block copies its rows to where the
// prefix sum of the sizes puts them
__global__ __launch_bounds__(256) void k_gather_sizes(const int32_t* __restrict__ ids, int64_t m,
                                                      const int32_t* __restrict__ blk_size, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = (uint32_t)blk_size[ids[i]];
}
__global__ __launch_bounds__(256) void k_gather_rows(const int32_t* __restrict__ ids, int64_t m,
                                                     const uint32_t* __restrict__ blk_start,
                                                     const int32_t* __restrict__ blk_size,
                                                     const uint32_t* __restrict__ offs, const double* __restrict__ xyz,
                                                     double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;
  const int32_t b = ids[i];
  const double* src = xyz + 3 * (size_t)blk_start[b];
  double* dst = out + 3 * (size_t)offs[i];
  const int n3 = 3 * blk_size[b];
  for (int j = threadIdx.x & 63; j < n3; j += 64) dst[j] = src[j];
}

}  // namespace

void forest_reset_scheme(octl_forest* f) {
  forest_forget_pending(f);   // (counts of a compaction still in flight: nobody will ask for them)
  f->max_block_hint = INT64_MAX;
  f->displaced_rows = false;
  f->store_dirty = true;
  f->nodes[0].n = f->nodes[1].n = 0;
  f->cur = 0;
  f->epoch = 0;
  f->built = false;
  f->vkeys.clear();
  f->vkeys_stale = false;
  f->vorg_set = false;
  f->vcode_valid = false;
  f->fast_order_valid = false;
  f->built_store = 0;
  f->built_poses = 0;
  f->append_only = true;
  f->n_voxels = 0;
  f->level_segs.clear();
  f->n_internal = 0;
  f->max_depth_reached = 0;
  f->n_ord = 0;
  f->n_blocks = 0;
  f->mask_valid = false;
  f->split_stats_valid = false;
  forest_contents_changed(f);
}

extern "C" {

int octl_forest_create(octl_ctx* ctx, int mode, const double corner[3], double edge,
                       octl_forest** out) {
  if (!ctx || !out || !corner) return OCTL_E_INVALID;
  *out = nullptr;
  if (mode != 0 && mode != 1) return octl_set_error(ctx, OCTL_E_INVALID, "mode must be 0 or 1");
  if (!(edge > 0.0)) return octl_set_error(ctx, OCTL_E_INVALID, "edge length must be positive");
  if (mode == 0) {
    if (corner[0] != 0.0 || corner[1] != 0.0 || corner[2] != 0.0)
      return octl_set_error(ctx, OCTL_E_INVALID,
                            "a non-zero grid corner is outside the parity domain: the reference "
                            "places its octrees relative to the corner but subtracts absolute "
                            "points (grid.py:96-105 vs octree.py:74)");
    if (edge != (double)(int64_t)edge)
      return octl_set_error(ctx, OCTL_E_INVALID,
                            "voxel_edge_length must be integer valued: the reference truncates "
                            "voxel coordinates with astype(int) (grid.py:72-76)");
  }
  octl_forest* f = new octl_forest();
  f->ctx = ctx;
  f->mode = mode;
  for (int a = 0; a < 3; ++a) f->corner[a] = corner[a];
  f->edge = edge;
  *out = f;
  return OCTL_OK;
}

void octl_forest_destroy(octl_forest* f) {
  if (!f) return;
  forest_forget_pending(f);
  if (f->ctx->ahead_forest == f) {  // (a forest at the same address later is another forest: its build is serial)
    f->ctx->ahead_forest = nullptr;
    f->ctx->ahead_mark_valid = f->ctx->ahead_mark_pending = false;
  }
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  nodes_free(f->ctx, f->nodes[0]);
  nodes_free(f->ctx, f->nodes[1]);
  if (f->store_borrowed) {  // (the caller's buffer is not ours to release)
    f->xyz = f->xyz_own;
    f->xyz_own = DevBuf{};
    f->store_borrowed = false;
  }
  for (DevBuf* b :
       {&f->bbox_dev, &f->part_xyz[0], &f->part_xyz[1], &f->bk_table, &f->bk_tot, &f->bk_chunks, &f->bk_vox, &f->bk_node, &f->leafinfo,
        &f->xyz, &f->alive, &f->alive2, &f->ord_idx, &f->xyz_ord, &f->pos_node, &f->blk_node, &f->blk_slot,
        &f->blk_start, &f->blk_size, &f->blk_node2, &f->blk_slot2, &f->blk_start2, &f->blk_size2, &f->mask, &f->blk_eval, &f->rs_scratch, &f->rs_order, &f->fast_order,
        &f->rs_hyp, &f->rs_plane, &f->rs_count, &f->rs_index, &f->ord_idx2, &f->xyz_ord2,
        &f->vkey, &f->path, &f->lin[0], &f->lin[1], &f->val[0], &f->val[1],
        &f->hist, &f->idxbuf[0], &f->idxbuf[1], &f->pathbuf[0], &f->pathbuf[1], &f->flags,
        &f->entries, &f->split[0], &f->split[1], &f->split_tiles[0], &f->split_tiles[1],
        &f->child_sc, &f->pose_off_dev, &f->scheme_dev, &f->root_up, &f->vlin_dev, &f->vcode_dev[0],
        &f->vcode_dev[1], &f->split_lambda, &f->split_n, &f->pl_rows, &f->pl_plane, &f->pl_node_row, &f->grp_scratch,
        &f->pl_hist, &f->q_stage, &f->rg_rows, &f->adj_tab, &f->adj_call, &f->nn_tab, &f->seg_tab, &f->seg_out,
        &f->seg_sort, &f->xf_tab})
    devbuf_release(f->ctx, *b);
  delete f;
}

int octl_forest_clear(octl_forest* f) {
  if (!f) return OCTL_E_INVALID;
  f->bbox_stale = true;   // (nothing is launched: whoever fills the box next resets it first)
  f->alive_stale = false;
  if (f->store_borrowed) {  // back to the forest's own block; the caller's buffer is the caller's again
    f->xyz = f->xyz_own;
    f->xyz_own = DevBuf{};
    f->store_borrowed = false;
  }
  f->bbox_pending = false;
  f->pose_off.assign(1, 0);
  f->n_store = f->n_alive = 0;
  forest_reset_scheme(f);
  return OCTL_OK;
}

// a build that failed half way has overwritten scratch the previous tables referred to: the forest is left WITHOUT
// a scheme (its points and voxels are kept); the next build starts from the top-level voxels again
static void forest_drop_scheme(octl_forest* f) {
  f->built = false;
  f->n_ord = 0;
  f->n_blocks = 0;
  f->n_internal = 0;
  f->mask_valid = false;
  f->store_dirty = true;
  f->split_stats_valid = false;
  forest_contents_changed(f);
}

int octl_forest_build(octl_forest* f, int64_t K, const uint8_t* scheme_mask, int32_t n_mask,
                      int32_t keep_scheme, int32_t max_depth, octl_build_info* info) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  const int64_t nodes_before = f->built ? f->nodes[f->cur].n : -1, voxels_before = f->n_voxels;
  const int rc = forest_build(f, K, scheme_mask, n_mask, keep_scheme, max_depth, info);
  if (rc != OCTL_OK && rc != OCTL_E_INVALID && rc != OCTL_E_STATE) forest_drop_scheme(f);
  // the split statistics of a planar build describe the node table it left: a placement into that scheme that adds
  // no voxel keeps the numbering (roots in voxel order, children in the order of their parents), anything else
  // renumbers or replaces the nodes
  if (rc == OCTL_OK && (!keep_scheme || f->nodes[f->cur].n != nodes_before || f->n_voxels != voxels_before))
    f->split_stats_valid = false;
  return rc;
}

int octl_forest_build_planar(octl_forest* f, int64_t K, double max_variance, int32_t min_points, int32_t ddof,
                             const uint8_t* scheme_mask, int32_t n_mask, int32_t max_depth, octl_build_info* info) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  // (max_variance > 0 is what bounds the depth: the statistic of points inside a cube of edge e is at most e^2 / 3)
  if (!(max_variance > 0.0) || !(max_variance <= 1.7976931348623157e308))
    return octl_set_error(ctx, OCTL_E_INVALID, "build_planar: max_variance must be finite and > 0 (got %g)",
                          max_variance);
  if (min_points < 4)
    return octl_set_error(ctx, OCTL_E_INVALID, "build_planar: min_points must be >= 4 (got %d)", min_points);
  if (ddof != 0 && ddof != 1)
    return octl_set_error(ctx, OCTL_E_INVALID, "build_planar: ddof must be 0 or 1 (got %d)", ddof);
  const PlanarRule rule{max_variance, min_points, ddof};
  f->split_stats_valid = false;
  const int rc = forest_build(f, K, scheme_mask, n_mask, 0, max_depth, info, &rule);
  if (rc != OCTL_OK && rc != OCTL_E_INVALID && rc != OCTL_E_STATE) forest_drop_scheme(f);
  return rc;
}

int octl_forest_set_scheme(octl_forest* f, const int32_t* first_child, const int32_t* epoch,
                           int64_t n_nodes, int32_t new_epoch) {
  if (!f || !first_child || !epoch) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "set_scheme needs a built forest");
  const int64_t V = f->n_voxels;
  if (n_nodes < V || (n_nodes - V) % 8 != 0 || n_nodes >= ((int64_t)1 << 31))
    return octl_set_error(ctx, OCTL_E_INVALID, "scheme must have V roots + 8 nodes per internal node");
  int64_t n_internal = 0;
  for (int64_t i = 0; i < n_nodes; ++i) {
    const int32_t c = first_child[i];
    if (c >= 0) {
      if (c < V || (int64_t)c + 8 > n_nodes || (c - V) % 8 != 0)
        return octl_set_error(ctx, OCTL_E_INVALID, "first_child[%lld] = %d is not a valid child group",
                              (long long)i, c);
      ++n_internal;
    }
  }
  if (V + 8 * n_internal != n_nodes)
    return octl_set_error(ctx, OCTL_E_INVALID, "node count does not match the number of internal nodes");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  NodeTable& t = f->nodes[f->cur];
  OCTL_TRY(nodes_reserve(ctx, t, n_nodes));
  HIP_TRY(ctx, hipMemcpyAsync(t.first_child.p, first_child, (size_t)n_nodes * 4, hipMemcpyHostToDevice,
                              ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(t.epoch.p, epoch, (size_t)n_nodes * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  t.n = n_nodes;
  f->n_internal = n_internal;
  f->uniform_epoch = false;
  f->split_stats_valid = false;
  forest_contents_changed(f);
  if (new_epoch > f->epoch) f->epoch = new_epoch;
  // only first_child / epoch of this table are meaningful until the next (keep_scheme) build,
  // which has to place every point again
  f->append_only = false;
  f->fast_order_valid = false;
  f->n_ord = 0;
  f->n_blocks = 0;
  f->mask_valid = false;
  return OCTL_OK;
}

int octl_forest_set_contents(octl_forest* f, int64_t n_blocks, const int32_t* blk_node, const int32_t* blk_slot,
                             const int32_t* blk_size, const double* xyz) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built || f->store_dirty)
    return octl_set_error(ctx, OCTL_E_STATE, "set_contents needs a forest whose tables are up to date (build first)");
  if (n_blocks < 0 || (n_blocks > 0 && (!blk_node || !blk_slot || !blk_size)))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad block arrays");
  const int n_poses = (int)f->pose_off.size() - 1;
  const int64_t n_nodes = f->nodes[f->cur].n;
  // new pose offsets: the store is pose-major, a pose's points in the storage order of its blocks
  std::vector<int64_t> per_slot((size_t)std::max(n_poses, 1), 0);
  int64_t total = 0;
  for (int64_t b = 0; b < n_blocks; ++b) {
    if (blk_size[b] <= 0) return octl_set_error(ctx, OCTL_E_INVALID, "block %lld is empty", (long long)b);
    if (blk_slot[b] < 0 || blk_slot[b] >= n_poses || blk_node[b] < 0 || blk_node[b] >= n_nodes)
      return octl_set_error(ctx, OCTL_E_INVALID, "block %lld: bad node or pose slot", (long long)b);
    per_slot[(size_t)blk_slot[b]] += blk_size[b];
    total += blk_size[b];
  }
  if (total >= ((int64_t)1 << 31)) return octl_set_error(ctx, OCTL_E_INVALID, "more than 2^31-1 points in one forest");
  if (total > 0 && !xyz) return octl_set_error(ctx, OCTL_E_INVALID, "null point array");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // The blocks must name LEAVES of the current scheme, every (leaf, pose) pair at most once, in the storage order
  // of the block table they replace: the (leaf, pose) pairs of the table this forest holds, some of them possibly
  // missing (emptied leaves), none added out of place.  A table that breaks this would be committed as it is and
  // corrupt every later query, so it is checked against the forest's own table first.
  if (n_blocks > 0) {
    std::vector<int32_t> fc((size_t)n_nodes);
    HIP_TRY(ctx, hipMemcpyAsync(fc.data(), f->nodes[f->cur].first_child.p, (size_t)n_nodes * 4, hipMemcpyDeviceToHost, st));
    const int64_t nb_old = f->n_blocks;
    std::vector<int32_t> on((size_t)std::max<int64_t>(nb_old, 1)), os((size_t)std::max<int64_t>(nb_old, 1));
    if (nb_old > 0) {
      HIP_TRY(ctx, hipMemcpyAsync(on.data(), f->blk_node.p, (size_t)nb_old * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipMemcpyAsync(os.data(), f->blk_slot.p, (size_t)nb_old * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // rank of a (leaf, pose) pair in the current table's storage order; pairs the table does not hold (a leaf that
    // was empty for the pose) sort by their leaf's first occurrence - unknown leaves keep the caller's order
    // among themselves only as far as (node, slot) is strictly increasing
    std::unordered_map<uint64_t, int64_t> rank;
    rank.reserve((size_t)nb_old * 2 + 1);
    for (int64_t b = 0; b < nb_old; ++b) rank.emplace(((uint64_t)(uint32_t)on[(size_t)b] << 32) | (uint32_t)os[(size_t)b], b);
    int64_t last_rank = -1;
    uint64_t last_unknown = 0;
    bool have_unknown = false;
    std::unordered_map<uint64_t, char> seen;
    seen.reserve((size_t)n_blocks * 2 + 1);
    for (int64_t b = 0; b < n_blocks; ++b) {
      if (fc[(size_t)blk_node[b]] >= 0)
        return octl_set_error(ctx, OCTL_E_INVALID, "block %lld: node %d is not a leaf of the scheme", (long long)b,
                              blk_node[b]);
      const uint64_t key = ((uint64_t)(uint32_t)blk_node[b] << 32) | (uint32_t)blk_slot[b];
      if (!seen.emplace(key, 1).second)
        return octl_set_error(ctx, OCTL_E_INVALID, "block %lld: (leaf %d, pose slot %d) appears twice", (long long)b,
                              blk_node[b], blk_slot[b]);
      const auto it = rank.find(key);
      if (it != rank.end()) {
        if (it->second <= last_rank)
          return octl_set_error(ctx, OCTL_E_INVALID,
                                "block %lld: (leaf %d, pose slot %d) is out of the storage order of the block table",
                                (long long)b, blk_node[b], blk_slot[b]);
        last_rank = it->second;
        have_unknown = false;
      } else {
        if (have_unknown && key <= last_unknown)
          return octl_set_error(ctx, OCTL_E_INVALID,
                                "block %lld: (leaf %d, pose slot %d) is out of order", (long long)b, blk_node[b], blk_slot[b]);
        last_unknown = key;
        have_unknown = true;
      }
    }
  }
  std::vector<int64_t> off((size_t)n_poses + 1, 0);
  for (int p = 0; p < n_poses; ++p) off[(size_t)p + 1] = off[(size_t)p] + per_slot[(size_t)p];
  std::vector<int64_t> cursor(off.begin(), off.end() - 1);
  std::vector<double> store((size_t)std::max<int64_t>(total, 1) * 3);
  std::vector<uint32_t> ord((size_t)std::max<int64_t>(total, 1)), starts((size_t)std::max<int64_t>(n_blocks, 1));
  int64_t pos = 0;
  for (int64_t b = 0; b < n_blocks; ++b) {
    starts[(size_t)b] = (uint32_t)pos;
    int64_t& c = cursor[(size_t)blk_slot[b]];
    std::memcpy(store.data() + 3 * c, xyz + 3 * pos, (size_t)blk_size[b] * 24);
    for (int32_t i = 0; i < blk_size[b]; ++i) ord[(size_t)(pos + i)] = (uint32_t)(c + i);
    c += blk_size[b];
    pos += blk_size[b];
  }
  // rows outside the cube of their leaf (the reference's test: floor((p - corner) / (edge / 2)) in {0, 1} per axis,
  // octree.py:73-75,94-98 - i.e. 0 <= p - corner < edge with the rounded difference)
  bool displaced = false;
  if (total > 0) {
    NodeTable& t = f->nodes[f->cur];
    std::vector<double> corner((size_t)n_nodes * 3), edge((size_t)n_nodes);
    HIP_TRY(ctx, hipMemcpyAsync(corner.data(), t.corner.p, (size_t)n_nodes * 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(edge.data(), t.edge.p, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    int64_t q = 0;
    for (int64_t b = 0; b < n_blocks && !displaced; ++b) {
      const double* c = corner.data() + 3 * (size_t)blk_node[b];
      const double e = edge[(size_t)blk_node[b]];
      for (int32_t i = 0; i < blk_size[b] && !displaced; ++i, ++q) {
        for (int a = 0; a < 3; ++a) {
          const double d = xyz[3 * q + a] - c[a];
          if (!(d >= 0.0 && d < e)) displaced = true;  // (also NaN)
        }
      }
      if (displaced) break;
    }
  }
  // The new store is the forest's own.  While the old one is BORROWED (the caller's buffer, never written) the
  // new points go to the forest's own block and the borrow ends only at the commit below; every allocation
  // comes before the first byte is overwritten, so that a failed allocation leaves the forest as it was.
  DevBuf& own = f->store_borrowed ? f->xyz_own : f->xyz;
  const size_t n1 = (size_t)std::max<int64_t>(total, 1), nb1 = (size_t)std::max<int64_t>(n_blocks, 1);
  OCTL_TRY(devbuf_reserve(ctx, own, n1 * 24 + 16));
  OCTL_TRY(devbuf_reserve(ctx, f->alive, n1 + 2));
  OCTL_TRY(devbuf_reserve(ctx, f->ord_idx, n1 * 4));
  OCTL_TRY(devbuf_reserve(ctx, f->xyz_ord, n1 * 24));
  // (block buffers keep the capacity convention of forest_make_blocks: one block per point)
  for (DevBuf* b : {&f->blk_node, &f->blk_slot, &f->blk_start, &f->blk_size})
    OCTL_TRY(devbuf_reserve(ctx, *b, std::max(n1, nb1) * 4));
  auto upload = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    auto up = [&](void* dst, const void* src, size_t bytes) {
      if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    };
    up(own.p, store.data(), (size_t)total * 24);
    up(f->xyz_ord.p, xyz, (size_t)total * 24);
    up(f->ord_idx.p, ord.data(), (size_t)total * 4);
    if (e == hipSuccess && total > 0) e = hipMemsetAsync(f->alive.p, 1, (size_t)total, st);
    up(f->blk_node.p, blk_node, (size_t)n_blocks * 4);
    up(f->blk_slot.p, blk_slot, (size_t)n_blocks * 4);
    up(f->blk_size.p, blk_size, (size_t)n_blocks * 4);
    up(f->blk_start.p, starts.data(), (size_t)n_blocks * 4);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // (pageable sources)
    return e;
  };
  if (const hipError_t e = upload(); e != hipSuccess) {
    // the tables (and an own store) are partly overwritten: the forest is left EMPTY but valid rather than
    // with sizes that describe arrays which no longer hold them
    (void)octl_forest_clear(f);
    return octl_set_error(ctx, OCTL_E_HIP, "set_contents: upload failed (%s); the forest was cleared",
                          hipGetErrorString(e));
  }
  // ---- commit ------------------------------------------------------------------------------------------------
  if (f->store_borrowed) {
    f->xyz = f->xyz_own;
    f->xyz_own = DevBuf{};
    f->store_borrowed = false;
  }
  f->pose_off = off;
  f->n_store = f->n_alive = f->n_ord = total;
  f->n_blocks = n_blocks;
  f->built_store = total;
  f->built_poses = n_poses;
  f->append_only = true;
  f->store_dirty = false;
  f->mask_valid = false;
  f->fast_order_valid = false;
  forest_contents_changed(f);
  // the voxel box of the new points is not known (rows may have left their cubes): the next build finds it
  f->max_block_hint = INT64_MAX;
  f->bbox_stale = true;
  f->alive_stale = false;   // (written above)
  f->bbox_pending = total > 0;
  f->displaced_rows = displaced;
  return OCTL_OK;
}

int octl_forest_get_nodes(octl_forest* f, int64_t cap, int32_t* voxel, int32_t* depth,
                          int32_t* parent, int32_t* first_child, double* corner, double* edge,
                          int32_t* epoch, int64_t* n_nodes) {
  if (!f || !n_nodes) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  NodeTable& t = f->nodes[f->cur];
  *n_nodes = t.n;
  const int64_t n = std::min<int64_t>(cap, t.n);
  if (n <= 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  auto dl = [&](void* dst, const DevBuf& src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  HIP_TRY(ctx, dl(voxel, t.voxel, (size_t)n * 4));
  HIP_TRY(ctx, dl(depth, t.depth, (size_t)n * 4));
  HIP_TRY(ctx, dl(parent, t.parent, (size_t)n * 4));
  HIP_TRY(ctx, dl(first_child, t.first_child, (size_t)n * 4));
  HIP_TRY(ctx, dl(corner, t.corner, (size_t)n * 24));
  HIP_TRY(ctx, dl(edge, t.edge, (size_t)n * 8));
  HIP_TRY(ctx, dl(epoch, t.epoch, (size_t)n * 4));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_get_voxels(octl_forest* f, int64_t cap, int64_t* coords, int64_t* n_voxels) {
  if (!f || !n_voxels) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  if (!f->built) return octl_set_error(f->ctx, OCTL_E_STATE, "no scheme has been built");
  *n_voxels = f->n_voxels;
  if (!coords) return OCTL_OK;
  OCTL_TRY(forest_sync_vkeys(f));
  const int64_t n = std::min<int64_t>(cap, *n_voxels);
  for (int64_t v = 0; v < n; ++v) {
    int64_t q[3];
    vkey_decode(f->vkeys[v], f->vorg, q);
    // the reference's voxel coordinates are int(q * L): the corner, not the index
    for (int a = 0; a < 3; ++a)
      coords[3 * v + a] = f->mode == 0 ? (int64_t)((double)q[a] * f->edge) : 0;
  }
  return OCTL_OK;
}

int octl_forest_get_blocks(octl_forest* f, int64_t cap, int32_t* node, int32_t* slot,
                           int64_t* start, int32_t* size, int64_t* n_blocks) {
  if (!f || !n_blocks) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  *n_blocks = f->n_blocks;
  const int64_t n = std::min<int64_t>(cap, f->n_blocks);
  if (n <= 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  if (node) HIP_TRY(ctx, hipMemcpyAsync(node, f->blk_node.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (slot) HIP_TRY(ctx, hipMemcpyAsync(slot, f->blk_slot.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (size) HIP_TRY(ctx, hipMemcpyAsync(size, f->blk_size.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (start) {
    OCTL_TRY(devbuf_reserve(ctx, f->rs_scratch, (size_t)n * 8));
    OCTL_LAUNCH(k_widen_u32_i64, dim3(grid_for(n)), dim3(256), 0, st,
                       (const uint32_t*)f->blk_start.as<uint32_t>(), n,
                       f->rs_scratch.as<int64_t>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(start, f->rs_scratch.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_get_slot_voxels(octl_forest* f, int32_t slot, int64_t cap, int32_t* voxel_ranks,
                                int64_t* n_out) {
  if (!f || !n_out) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  const int n_poses = (int)f->pose_off.size() - 1;
  if (slot < 0 || slot >= n_poses) return octl_set_error(ctx, OCTL_E_INVALID, "bad pose slot");
  *n_out = 0;
  const int64_t V = f->n_voxels, nb = f->n_blocks;
  if (V <= 0 || nb <= 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  // scratch inside rs_scratch: [flags u32 V+8 | scanned u32 V+8 | out i32 V]
  const size_t seg = (((size_t)V + 8) * 4 + 15) & ~(size_t)15;
  OCTL_TRY(devbuf_reserve(ctx, f->rs_scratch, 3 * seg));
  char* base = static_cast<char*>(f->rs_scratch.p);
  uint32_t* flags = reinterpret_cast<uint32_t*>(base);
  uint32_t* scanned = reinterpret_cast<uint32_t*>(base + seg);
  int32_t* out = reinterpret_cast<int32_t*>(base + 2 * seg);
  uint32_t* total = ctx->small.as<uint32_t>() + SM_SLOT_VOXELS;
  HIP_TRY(ctx, hipMemsetAsync(flags, 0, seg, st));
  OCTL_LAUNCH(k_slot_voxel_flags, dim3(grid_for(nb)), dim3(256), 0, st,
                     (const int32_t*)f->blk_node.as<int32_t>(), (const int32_t*)f->blk_slot.as<int32_t>(),
                     nb, slot, (const int32_t*)f->nodes[f->cur].voxel.as<int32_t>(), flags);
  HIP_TRY(ctx, hipGetLastError());
  OCTL_TRY(octl_exclusive_scan_u32(ctx, flags, scanned, V, total));
  OCTL_LAUNCH(k_flag_indices, dim3(grid_for(V)), dim3(256), 0, st, (const uint32_t*)flags,
                     (const uint32_t*)scanned, V, out);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t cnt;
  OCTL_TRY(octl_readback(ctx, total, 1, &cnt));
  *n_out = cnt;
  const int64_t m = std::min<int64_t>(cap, cnt);
  if (m > 0 && voxel_ranks) {
    HIP_TRY(ctx, hipMemcpyAsync(voxel_ranks, out, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return OCTL_OK;
}

int octl_forest_slot_counts(octl_forest* f, int32_t slot, int64_t* n_points, int64_t* n_leaves) {
  if (!f || !n_points || !n_leaves) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  const int n_poses = (int)f->pose_off.size() - 1;
  if (slot < 0 || slot >= n_poses) return octl_set_error(ctx, OCTL_E_INVALID, "bad pose slot");
  *n_points = *n_leaves = 0;
  if (f->n_blocks <= 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(ctx->small.as<uint32_t>() + SM_SLOT_COUNTS);
  HIP_TRY(ctx, hipMemsetAsync(out, 0, 16, st));
  OCTL_LAUNCH(k_slot_counts, dim3((unsigned)std::min<int64_t>(1024, ceil_div(f->n_blocks, 256))), dim3(256),
                     0, st, (const int32_t*)f->blk_slot.as<int32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                     f->n_blocks, slot, out);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long r[2];
  OCTL_TRY(octl_readback(ctx, out, 4, r));
  *n_points = (int64_t)r[0];
  *n_leaves = (int64_t)r[1];
  return OCTL_OK;
}

int octl_forest_internal_per_voxel(octl_forest* f, int64_t cap, int32_t* counts, int64_t* n_voxels) {
  if (!f || !n_voxels) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  *n_voxels = f->n_voxels;
  const int64_t V = std::min<int64_t>(cap, f->n_voxels);
  if (V <= 0 || !counts) return OCTL_OK;
  hipStream_t st = ctx->stream;
  NodeTable& t = f->nodes[f->cur];
  OCTL_TRY(devbuf_reserve(ctx, f->rs_scratch, (size_t)f->n_voxels * 4));
  HIP_TRY(ctx, hipMemsetAsync(f->rs_scratch.p, 0, (size_t)f->n_voxels * 4, st));
  OCTL_LAUNCH(k_internal_per_voxel, dim3(grid_for(t.n)), dim3(256), 0, st,
                     (const int32_t*)t.first_child.as<int32_t>(), (const int32_t*)t.voxel.as<int32_t>(), t.n,
                     f->rs_scratch.as<int32_t>());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(counts, f->rs_scratch.p, (size_t)V * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_get_perm(octl_forest* f, int64_t cap, int64_t* perm, int64_t* n_out) {
  if (!f || !n_out) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  *n_out = f->n_ord;
  const int64_t n = std::min<int64_t>(cap, f->n_ord);
  if (n <= 0 || !perm) return OCTL_OK;
  hipStream_t st = ctx->stream;
  OCTL_TRY(devbuf_reserve(ctx, f->rs_scratch, (size_t)n * 8));
  OCTL_LAUNCH(k_widen_u32_i64, dim3(grid_for(n)), dim3(256), 0, st,
                     (const uint32_t*)f->ord_idx.as<uint32_t>(), n, f->rs_scratch.as<int64_t>());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(perm, f->rs_scratch.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_get_points(octl_forest* f, int64_t start, int64_t count, double* xyz) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  if (start < 0 || count < 0 || start + count > f->n_ord)
    return octl_set_error(ctx, OCTL_E_INVALID, "point range out of bounds");
  if (count == 0) return OCTL_OK;
  if (!xyz) return OCTL_E_INVALID;
  HIP_TRY(ctx, hipMemcpyAsync(xyz, f->xyz_ord.as<double>() + 3 * start, (size_t)count * 24,
                              hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OCTL_OK;
}

int octl_forest_gather_blocks(octl_forest* f, const int32_t* block_ids, int64_t m, int64_t cap, double* xyz,
                              int64_t* n_points) {
  if (!f || !n_points || m < 0 || (m > 0 && !block_ids)) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  *n_points = 0;
  if (m == 0) return OCTL_OK;
  for (int64_t i = 0; i < m; ++i)
    if (block_ids[i] < 0 || block_ids[i] >= f->n_blocks) return octl_set_error(ctx, OCTL_E_INVALID, "bad block id");
  hipStream_t st = ctx->stream;
  // scratch (f->hist): [ids i32 m | sizes -> offsets u32 m + 1 | total]
  const size_t o_sz = (((size_t)m * 4) + 15) & ~(size_t)15;
  const size_t o_tot = o_sz + ((((size_t)m + 1) * 4) + 15) / 16 * 16;
  OCTL_TRY(devbuf_reserve(ctx, f->hist, o_tot + 16));
  char* base = static_cast<char*>(f->hist.p);
  int32_t* ids_d = reinterpret_cast<int32_t*>(base);
  uint32_t* offs = reinterpret_cast<uint32_t*>(base + o_sz);
  uint32_t* total = reinterpret_cast<uint32_t*>(base + o_tot);
  HIP_TRY(ctx, hipMemcpyAsync(ids_d, block_ids, (size_t)m * 4, hipMemcpyHostToDevice, st));
  OCTL_LAUNCH(k_gather_sizes, dim3(grid_for(m)), dim3(256), 0, st, (const int32_t*)ids_d, m,
                     (const int32_t*)f->blk_size.as<int32_t>(), offs);
  HIP_TRY(ctx, hipGetLastError());
  OCTL_TRY(octl_exclusive_scan_u32(ctx, offs, offs, m, total));
  uint32_t tot_h = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&tot_h, total, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (also: the pageable id list is the caller's again)
  *n_points = tot_h;
  if (tot_h == 0 || !xyz || cap < (int64_t)tot_h) return OCTL_OK;  // (size query, or nothing to copy)
  // the gathered rows go through the compaction target of apply_mask (free between calls)
  OCTL_TRY(devbuf_reserve(ctx, f->xyz_ord2, (size_t)tot_h * 24));
  OCTL_LAUNCH(k_gather_rows, dim3((unsigned)ceil_div(m, 4)), dim3(256), 0, st, (const int32_t*)ids_d, m,
                     (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                     (const uint32_t*)offs, (const double*)f->xyz_ord.as<double>(), f->xyz_ord2.as<double>());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(xyz, f->xyz_ord2.p, (size_t)tot_h * 24, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_ransac(octl_forest* f, const int32_t* block_order, int64_t nb,
                       const double* hypotheses, int32_t H, int32_t k, double threshold,
                       float* plane, int32_t* best_count, int32_t* best_index) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "ransac before build");
  if (nb < 0 || (nb > 0 && !block_order) || !hypotheses)
    return octl_set_error(ctx, OCTL_E_INVALID, "bad ransac arguments");
  if (H < 1 || H > 1024 || k < 1) return octl_set_error(ctx, OCTL_E_INVALID, "bad H or k");
  OCTL_TRY(ransac_check_table(ctx, hypotheses, H, k));
  for (int64_t b = 0; b < nb; ++b)
    if (block_order[b] < 0 || block_order[b] >= f->n_blocks)
      return octl_set_error(ctx, OCTL_E_INVALID, "block index out of range");
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  OCTL_TRY(ensure_mask(f));
  if (nb == 0) return OCTL_OK;
  OCTL_TRY(devbuf_reserve(ctx, f->rs_order, (size_t)nb * 4));
  OCTL_TRY(devbuf_reserve(ctx, f->rs_hyp, (size_t)H * k * 8));
  HIP_TRY(ctx, hipMemcpyAsync(f->rs_order.p, block_order, (size_t)nb * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(f->rs_hyp.p, hypotheses, (size_t)H * k * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  float* plane_d = nullptr;
  int32_t *count_d = nullptr, *index_d = nullptr;
  if (plane) {
    OCTL_TRY(devbuf_reserve(ctx, f->rs_plane, (size_t)nb * 16));
    plane_d = f->rs_plane.as<float>();
  }
  if (best_count) {
    OCTL_TRY(devbuf_reserve(ctx, f->rs_count, (size_t)nb * 4));
    count_d = f->rs_count.as<int32_t>();
  }
  if (best_index) {
    OCTL_TRY(devbuf_reserve(ctx, f->rs_index, (size_t)nb * 4));
    index_d = f->rs_index.as<int32_t>();
  }
  OCTL_TRY(ransac_launch(ctx, f->xyz_ord.as<double>(), f->n_ord, f->blk_start.as<uint32_t>(),
                         f->blk_size.as<int32_t>(), f->rs_order.as<int32_t>(), nb,
                         f->rs_hyp.as<double>(), H, k, threshold, f->mask.as<uint8_t>(), plane_d,
                         count_d, index_d, nullptr, f->rs_scratch, f->max_block_hint));
  if (plane) HIP_TRY(ctx, hipMemcpyAsync(plane, plane_d, (size_t)nb * 16, hipMemcpyDeviceToHost, st));
  if (best_count) HIP_TRY(ctx, hipMemcpyAsync(best_count, count_d, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
  if (best_index) HIP_TRY(ctx, hipMemcpyAsync(best_index, index_d, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_ransac_evaluate(octl_ctx* ctx, const double* point_cloud, int64_t M,
                         const int32_t* block_sizes, int64_t B, const double* hypotheses,
                         int32_t H, int32_t k, double threshold, uint8_t* mask_out,
                         float* planes_out, int32_t* best_count_out, int32_t* best_index_out) {
  if (!ctx) return OCTL_E_INVALID;
  if (M < 0 || B < 0 || (M > 0 && !point_cloud) || (B > 0 && !block_sizes) || !hypotheses ||
      (M > 0 && !mask_out))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad ransac_evaluate arguments");
  if (H < 1 || H > 1024 || k < 1) return octl_set_error(ctx, OCTL_E_INVALID, "bad H or k");
  OCTL_TRY(ransac_check_table(ctx, hypotheses, H, k));
  if (M >= ((int64_t)1 << 31)) return octl_set_error(ctx, OCTL_E_INVALID, "cloud too large");
  int64_t total = 0;
  std::vector<uint32_t> starts((size_t)std::max<int64_t>(B, 1));
  for (int64_t b = 0; b < B; ++b) {
    if (block_sizes[b] < 0) return octl_set_error(ctx, OCTL_E_INVALID, "negative block size");
    starts[b] = (uint32_t)total;  // np.cumsum([0] + sizes[:-1]) (cuda_ransac.py:64-66)
    total += block_sizes[b];
  }
  if (total > M)
    return octl_set_error(ctx, OCTL_E_INVALID, "block sizes add up to %lld > %lld points",
                          (long long)total, (long long)M);
  if (M == 0) return OCTL_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf xyz, sizes, starts_d, hyp, mask, plane, count, index, scratch;
  int rc = OCTL_OK;
  auto cleanup = [&]() {
    // (back to the context's pool, not to the allocator: hipFree synchronises the device, and the next
    //  evaluate() of a loop over batches wants the same blocks again)
    (void)hipStreamSynchronize(st);
    for (DevBuf* b : {&xyz, &sizes, &starts_d, &hyp, &mask, &plane, &count, &index, &scratch})
      devbuf_release(ctx, *b);
  };
#define EV_TRY(expr)            \
  do {                          \
    rc = (expr);                \
    if (rc != OCTL_OK) {        \
      cleanup();                \
      return rc;                \
    }                           \
  } while (0)
#define EV_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      cleanup();                                                                            \
      return octl_set_error(ctx, OCTL_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    }                                                                                       \
  } while (0)
  EV_TRY(devbuf_reserve(ctx, xyz, (size_t)M * 24));
  EV_TRY(devbuf_reserve(ctx, mask, (size_t)M));
  EV_TRY(devbuf_reserve(ctx, hyp, (size_t)H * k * 8));
  EV_HIP(hipMemcpyAsync(xyz.p, point_cloud, (size_t)M * 24, hipMemcpyHostToDevice, st));
  EV_HIP(hipMemcpyAsync(hyp.p, hypotheses, (size_t)H * k * 8, hipMemcpyHostToDevice, st));
  EV_HIP(hipMemsetAsync(mask.p, 0, (size_t)M, st));  // np.zeros (cuda_ransac.py:57)
  if (B > 0) {
    EV_TRY(devbuf_reserve(ctx, sizes, (size_t)B * 4));
    EV_TRY(devbuf_reserve(ctx, starts_d, (size_t)B * 4));
    EV_HIP(hipMemcpyAsync(sizes.p, block_sizes, (size_t)B * 4, hipMemcpyHostToDevice, st));
    EV_HIP(hipMemcpyAsync(starts_d.p, starts.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (planes_out) EV_TRY(devbuf_reserve(ctx, plane, (size_t)B * 16));
    if (best_count_out) EV_TRY(devbuf_reserve(ctx, count, (size_t)B * 4));
    if (best_index_out) EV_TRY(devbuf_reserve(ctx, index, (size_t)B * 4));
    EV_HIP(hipStreamSynchronize(st));
    int64_t max_size = 0;   // (the caller's block sizes are host data: the largest one is known)
    for (int64_t b = 0; b < B; ++b) max_size = std::max<int64_t>(max_size, block_sizes[b]);
    EV_TRY(ransac_launch(ctx, xyz.as<double>(), M, starts_d.as<uint32_t>(), sizes.as<int32_t>(),
                         nullptr, B, hyp.as<double>(), H, k, threshold, mask.as<uint8_t>(),
                         planes_out ? plane.as<float>() : nullptr,
                         best_count_out ? count.as<int32_t>() : nullptr,
                         best_index_out ? index.as<int32_t>() : nullptr, nullptr, scratch, max_size));
    if (planes_out) EV_HIP(hipMemcpyAsync(planes_out, plane.p, (size_t)B * 16, hipMemcpyDeviceToHost, st));
    if (best_count_out) EV_HIP(hipMemcpyAsync(best_count_out, count.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    if (best_index_out) EV_HIP(hipMemcpyAsync(best_index_out, index.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
  }
  EV_HIP(hipMemcpyAsync(mask_out, mask.p, (size_t)M, hipMemcpyDeviceToHost, st));
  EV_HIP(hipStreamSynchronize(st));
  cleanup();
#undef EV_TRY
#undef EV_HIP
  return OCTL_OK;
}

}  // extern "C"

// ---- test hooks for the device-wide primitives (tests/test_gpu_primitives.py) ----------------
extern "C" int octl_debug_exclusive_scan(octl_ctx* ctx, const uint32_t* in, int64_t n,
                                         uint32_t* out, uint32_t* total) {
  if (!ctx || n < 0 || (n > 0 && (!in || !out))) return OCTL_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf buf;
  OCTL_TRY(devbuf_reserve(ctx, buf, (size_t)(n + 8) * 4));
  hipStream_t st = ctx->stream;
  uint32_t* tot_d = ctx->small.as<uint32_t>() + SM_DEBUG_TOTAL;
  int rc = OCTL_OK;
  if (n > 0 && hipMemcpyAsync(buf.p, in, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = OCTL_E_HIP;
  if (rc == OCTL_OK) rc = octl_exclusive_scan_u32(ctx, buf.as<uint32_t>(), buf.as<uint32_t>(), n, tot_d);
  if (rc == OCTL_OK && n > 0 &&
      hipMemcpyAsync(out, buf.p, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = OCTL_E_HIP;
  if (rc == OCTL_OK && total &&
      hipMemcpyAsync(total, tot_d, 4, hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = OCTL_E_HIP;
  if (hipStreamSynchronize(st) != hipSuccess) rc = OCTL_E_HIP;
  devbuf_free(buf);
  return rc;
}

extern "C" int octl_debug_radix_sort(octl_ctx* ctx, uint64_t* keys, uint32_t* vals, int64_t n,
                                     int key_bits) {
  if (!ctx || n < 0 || (n > 0 && (!keys || !vals))) return OCTL_E_INVALID;
  if (n == 0) return OCTL_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf k[2], v[2], hist;
  int rc = OCTL_OK;
  for (int b = 0; b < 2 && rc == OCTL_OK; ++b) {
    rc = devbuf_reserve(ctx, k[b], (size_t)n * 8);
    if (rc == OCTL_OK) rc = devbuf_reserve(ctx, v[b], (size_t)n * 4);
  }
  if (rc == OCTL_OK) {
    if (hipMemcpyAsync(k[0].p, keys, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(v[0].p, vals, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      rc = OCTL_E_HIP;
  }
  int res = 0;
  if (rc == OCTL_OK) {
    uint64_t* kk[2] = {k[0].as<uint64_t>(), k[1].as<uint64_t>()};
    uint32_t* vv[2] = {v[0].as<uint32_t>(), v[1].as<uint32_t>()};
    rc = octl_radix_sort_u64_u32(ctx, kk, vv, n, key_bits, hist, &res);
  }
  if (rc == OCTL_OK) {
    if (hipMemcpyAsync(keys, k[res].p, (size_t)n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(vals, v[res].p, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      rc = OCTL_E_HIP;
  }
  for (int b = 0; b < 2; ++b) {
    devbuf_free(k[b]);
    devbuf_free(v[b]);
  }
  devbuf_free(hist);
  return rc;
}
