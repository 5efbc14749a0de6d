// Which stored points form one object: Euclidean cluster extraction - the connected components of "two stored points
// are within a radius of each other" - octl_forest_cluster_points, and the map-cleaning step made of it,
// octl_forest_remove_small_clusters.  Defined by octreelib_amd/clustering.py: cluster_labels_np and
// small_cluster_keep_np, and compared with them integer for integer.  No reference counterpart: the reference has no
// query across leaves.
//
//   vertices  the points of the ordered arrays that belong to a selected pose (alive; a pending RANSAC mask is not read);
//   edge      d2 = (dx dx + dy dy) + dz dz <= r2 = radius^2 in f64, products and sums separate and in that order
//             (-ffp-contract=off), inclusive: the candidates of octl_forest_radius_count, found by the same walk
//             (nearest_walk.h) over the block index of the SAME selection - every offered position is a vertex.
//
// The union-find (union_find.h) runs over positions of the ordered arrays.  Kernels of a call, in stream order:
//   k_cluster_init     one wavefront per (leaf, pose) block: parent[pos] = pos in a block of a selected pose, -1
//                      otherwise; size = 0, first = all ones; the error word and the row counter cleared
//   k_cluster_link     the self-query of k_sparse_mask: one wavefront per block of a selected pose, lanes striding over
//                      its positions, q = the stored bits; the sink (cluster_link.h) unites `self` with every offered
//                      position below it
//   k_cluster_flatten  per vertex: root -> parent[pos]; size[root] += 1; first[root] = min(slot << 32 | index)
//   k_cluster_rows     (cluster_points) one row per vertex {slot, index, first[root], size[root]}, a wave booking the
//                      rows of its block with one integer atomicAdd as k_point_stats does - the host orders them
//   k_cluster_mask     (remove_small_clusters) mask[pos] = 0 where size[root] < min_points, with the fill convention of
//                      k_sparse_mask; then the ONE compaction (mask.hip: mask_apply)
// Integer atomics only: the root of a component is its smallest position whatever the schedule (union_find.h), sums
// and minima of integers do not depend on their order.  No LDS, no scratch, no floating-point atomics; nothing is sized
// by the CU count.  Tables: 16 bytes per ordered point (parent i32, size u32, first u64) in f->grp_scratch.
#include <algorithm>
#include <climits>
#include <cmath>

#include "cluster_link.h"
#include "common.h"
#include "forest.h"

namespace {

// words behind the tables
enum { CL_W_ERR = 0, CL_W_WORDS = 4 };

struct ClusterTables {
  int32_t* parent;             // [n_ord]
  uint32_t* size;              // [n_ord] members of the component, at its root
  unsigned long long* first;   // [n_ord] smallest slot << 32 | index of the component, at its root
  uint32_t* words;             // [CL_W_WORDS]
  const uint32_t* pose_off;    // [poses] store offset of every pose
  const uint8_t* slot_sel;     // [poses], nullptr: every pose
};

struct BlockTable {
  const uint32_t* start;
  const int32_t* size;
  const int32_t* slot;
  int64_t nb;
};

// the (leaf, pose) block of this wavefront; false: none, or (selected_only) one of a pose that is not selected
__device__ __forceinline__ bool cluster_block(const BlockTable& B, const ClusterTables& C, bool selected_only,
                                              int64_t* s0, int64_t* n, int32_t* slot, bool* selected) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B.nb) return false;
  *slot = B.slot[b];
  *selected = !C.slot_sel || C.slot_sel[*slot] != 0;
  *s0 = B.start[b];
  *n = B.size[b];
  return *selected || !selected_only;
}

__global__ __launch_bounds__(256) void k_cluster_init(BlockTable B, ClusterTables C,
                                                      unsigned long long* __restrict__ n_rows) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    C.words[CL_W_ERR] = 0;
    if (n_rows) *n_rows = 0;
  }
  int64_t s0, n;
  int32_t slot;
  bool selected;
  if (!cluster_block(B, C, false, &s0, &n, &slot, &selected)) return;
  for (int64_t i = threadIdx.x & 63; i < n; i += 64) {
    const int64_t pos = s0 + i;
    C.parent[pos] = selected ? (int32_t)pos : -1;
    C.size[pos] = 0;
    C.first[pos] = ~0ull;
  }
}

__global__ __launch_bounds__(256) void k_cluster_link(BlockTable B, ClusterTables C, double r, double r2, NNTables T,
                                                      int64_t max_steps) {
  int64_t s0, n;
  int32_t slot;
  bool selected;
  if (!cluster_block(B, C, true, &s0, &n, &slot, &selected)) return;
  for (int64_t i = threadIdx.x & 63; i < n; i += 64)
    if (!cluster_link_one(T, C.parent, (int32_t)(s0 + i), r, r2, max_steps)) atomicOr(C.words + CL_W_ERR, 1u);
}

__global__ __launch_bounds__(256) void k_cluster_flatten(BlockTable B, ClusterTables C,
                                                         const uint32_t* __restrict__ ord_idx, int64_t max_steps) {
  int64_t s0, n;
  int32_t slot;
  bool selected;
  if (!cluster_block(B, C, true, &s0, &n, &slot, &selected)) return;
  const uint32_t off = C.pose_off[slot];
  for (int64_t i = threadIdx.x & 63; i < n; i += 64) {
    const int64_t pos = s0 + i;
    int64_t budget = max_steps;
    const int32_t root = uf_find(C.parent, (int32_t)pos, budget);
    if (root < 0) {
      atomicOr(C.words + CL_W_ERR, 1u);
      continue;
    }
    uf_lower(C.parent + pos, root);  // (its final value: nothing is below the root)
    atomicAdd(C.size + root, 1u);
    atomicMin(C.first + root, ((unsigned long long)(uint32_t)slot << 32) | (unsigned long long)(ord_idx[pos] - off));
  }
}

struct ClusterRows {
  int32_t* slot;
  int32_t* index;
  unsigned long long* first;
  uint32_t* size;
};

// cap: rows the table holds - the host's bound of the vertices; a block that would not fit writes nothing (and *n_rows
// then exceeds cap, which the host refuses)
__global__ __launch_bounds__(256) void k_cluster_rows(BlockTable B, ClusterTables C,
                                                      const uint32_t* __restrict__ ord_idx, int64_t n_ord, int64_t cap,
                                                      unsigned long long* __restrict__ n_rows, ClusterRows out) {
  int64_t s0, n;
  int32_t slot;
  bool selected;
  if (!cluster_block(B, C, true, &s0, &n, &slot, &selected) || n <= 0) return;
  const int lane = threadIdx.x & 63;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(n_rows, (unsigned long long)n);
  base = __shfl(base, 0);
  if ((int64_t)base + n > cap) return;
  const uint32_t off = C.pose_off[slot];
  for (int64_t i = lane; i < n; i += 64) {
    const int64_t pos = s0 + i, row = (int64_t)base + i;
    const int32_t root = C.parent[pos];
    const bool ok = root >= 0 && root < n_ord;  // (false only behind a set error word: the call fails)
    out.slot[row] = slot;
    out.index[row] = (int32_t)(ord_idx[pos] - off);
    out.first[row] = ok ? C.first[root] : ~0ull;
    out.size[row] = ok ? C.size[root] : 0u;
  }
}

// fill: no mask is pending, so every byte of every block is written here - 1 for what stays, the blocks of the poses
// that are not selected included - instead of in a fill launch (k_sparse_mask does the same).  Otherwise only zeros are
// written, and a pending RANSAC mask stays in the bytes.  Behind a set error word nothing is cleared: the call fails.
__global__ __launch_bounds__(256) void k_cluster_mask(BlockTable B, ClusterTables C, int64_t n_ord, uint32_t min_points,
                                                      int fill, uint8_t* __restrict__ mask) {
  int64_t s0, n;
  int32_t slot;
  bool selected;
  if (!cluster_block(B, C, !fill, &s0, &n, &slot, &selected)) return;
  const bool judge = selected && C.words[CL_W_ERR] == 0;
  for (int64_t i = threadIdx.x & 63; i < n; i += 64) {
    const int64_t pos = s0 + i;
    bool keep = true;
    if (judge) {
      const int32_t root = C.parent[pos];
      keep = !(root >= 0 && root < n_ord) || C.size[root] >= min_points;
    }
    if (fill) mask[pos] = keep ? 1 : 0;
    else if (!keep) mask[pos] = 0;
  }
}

// f->grp_scratch of a call: [parent i32 | size u32 | first u64 | words | store offsets u32 per pose | selection u8]
struct ClusterLayout {
  size_t n, poses;
  Carve plan;
  Carve::Part<int32_t> parent = plan.add<int32_t>(n);
  Carve::Part<uint32_t> size = plan.add<uint32_t>(n);
  Carve::Part<unsigned long long> first = plan.add<unsigned long long>(n);
  Carve::Part<uint32_t> words = plan.add<uint32_t>(CL_W_WORDS), off = plan.add<uint32_t>(poses);
  Carve::Part<uint8_t> sel = plan.add<uint8_t>(poses);
  ClusterLayout(int64_t n_ord, size_t n_poses) : n((size_t)std::max<int64_t>(n_ord, 1)), poses(std::max<size_t>(n_poses, 1)) {}
};

// f->q_stage of octl_forest_cluster_points for c rows: [slot i32 | index i32 | first u64 | size u32 | rows u64]
struct ClusterStage {
  size_t c;
  Carve plan;
  Carve::Part<int32_t> slot = plan.add<int32_t>(c), index = plan.add<int32_t>(c);
  Carve::Part<unsigned long long> first = plan.add<unsigned long long>(c);
  Carve::Part<uint32_t> size = plan.add<uint32_t>(c);
  Carve::Part<unsigned long long> rows = plan.add<unsigned long long>(1);
  explicit ClusterStage(int64_t rows_) : c((size_t)std::max<int64_t>(rows_, 1)) {}
};

// What both entries run: the tables reserved and their small uploads enqueued (`off32` and `sel` stay the caller's until
// the call's wait), then init, link and flatten.  T: the walk over the block index of `sel`.
int cluster_components(octl_forest* f, const NNTables& T, double radius,
                       const std::vector<uint8_t>& sel, std::vector<uint32_t>& off32, unsigned long long* rows_d,
                       BlockTable* B, ClusterTables* C) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const size_t n_poses = f->pose_off.size() - 1;
  const ClusterLayout lay(f->n_ord, n_poses);
  OCTL_TRY(devbuf_reserve(ctx, f->grp_scratch, lay.plan.total));
  DevBuf& g = f->grp_scratch;
  uint32_t* off_d = Carve::at(g, lay.off);
  uint8_t* sel_d = sel.empty() ? nullptr : Carve::at(g, lay.sel);
  off32.resize(n_poses);
  for (size_t s = 0; s < n_poses; ++s) off32[s] = (uint32_t)f->pose_off[s];  // (store indices are u32)
  if (n_poses) HIP_TRY(ctx, hipMemcpyAsync(off_d, off32.data(), n_poses * 4, hipMemcpyHostToDevice, st));
  if (sel_d) HIP_TRY(ctx, hipMemcpyAsync(sel_d, sel.data(), sel.size(), hipMemcpyHostToDevice, st));
  *B = BlockTable{f->blk_start.as<uint32_t>(), f->blk_size.as<int32_t>(), f->blk_slot.as<int32_t>(), f->n_blocks};
  *C = ClusterTables{Carve::at(g, lay.parent), Carve::at(g, lay.size), Carve::at(g, lay.first),
                     Carve::at(g, lay.words),  off_d,                  sel_d};
  // more steps than a sound table lets one union take (union_find.h: fewer than 3 n)
  const int64_t max_steps = 8 * f->n_ord + 64;
  const dim3 grid((unsigned)ceil_div(f->n_blocks, 4));
  {
    KTimer t(ctx, "cluster_init");
    OCTL_LAUNCH(k_cluster_init, grid, dim3(256), 0, st, *B, *C, rows_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  {
    KTimer t(ctx, "cluster_link");
    OCTL_LAUNCH(k_cluster_link, grid, dim3(256), 0, st, *B, *C, radius, radius * radius, T, max_steps);
    HIP_TRY(ctx, hipGetLastError());
  }
  {
    KTimer t(ctx, "cluster_flatten");
    OCTL_LAUNCH(k_cluster_flatten, grid, dim3(256), 0, st, *B, *C, (const uint32_t*)f->ord_idx.as<uint32_t>(),
                max_steps);
    HIP_TRY(ctx, hipGetLastError());
  }
  return OCTL_OK;
}

int cluster_budget_error(octl_ctx* ctx, const char* what) {
  return octl_set_error(ctx, OCTL_E_STATE, "%s: the union-find ran out of its step budget (damaged tables)", what);
}

}  // namespace

extern "C" {

int octl_forest_cluster_points(octl_forest* f, double radius, const uint8_t* slot_sel, int32_t n_sel, int64_t cap,
                               int64_t* n_rows, int32_t* slot, int32_t* index, int64_t* first, int32_t* size) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  if (f->built) {
    if (cap < 0 || !n_rows) return octl_set_error(ctx, OCTL_E_INVALID, "bad cluster arguments");
    OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  }
  // (the walk is asked for one query when there is a point to link: the index is made for the selection, and not at
  //  all for a map without ordered points)
  const bool some = f->n_ord > 0 && f->n_blocks > 0;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "cluster", some ? 1 : 0, 1, radius, slot_sel, n_sel, true, &T));
  *n_rows = 0;
  if (!some) return OCTL_OK;
  // the host's bound of the rows: the selected poses' rows of the store, and never more than the ordered points
  int64_t bound = 0;
  const size_t n_poses = f->pose_off.size() - 1;
  for (size_t s = 0; s < n_poses; ++s)
    if (sel.empty() || sel[s]) bound += f->pose_off[s + 1] - f->pose_off[s];
  bound = std::min(bound, f->n_ord);
  if (bound == 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  const ClusterStage lay(bound);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, lay.plan.total));
  DevBuf& q = f->q_stage;
  unsigned long long* rows_d = Carve::at(q, lay.rows);
  std::vector<uint32_t> off32;
  BlockTable B;
  ClusterTables C;
  OCTL_TRY(cluster_components(f, T, radius, sel, off32, rows_d, &B, &C));
  {
    KTimer t(ctx, "cluster_rows");
    OCTL_LAUNCH(k_cluster_rows, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st, B, C,
                (const uint32_t*)f->ord_idx.as<uint32_t>(), f->n_ord, bound, rows_d,
                ClusterRows{Carve::at(q, lay.slot), Carve::at(q, lay.index), Carve::at(q, lay.first),
                            Carve::at(q, lay.size)});
    HIP_TRY(ctx, hipGetLastError());
  }
  // one wait when the caller's arrays are known to hold every row (cap >= bound); otherwise the count first
  unsigned long long total = 0;
  uint32_t err = 0;
  const bool sure = cap >= bound;
  auto fetch = [&](size_t rows) -> int {
    bool any = false;
    HIP_TRY(ctx, octl_download(ctx, slot, q, lay.slot, rows, &any));
    HIP_TRY(ctx, octl_download(ctx, index, q, lay.index, rows, &any));
    HIP_TRY(ctx, octl_download(ctx, reinterpret_cast<unsigned long long*>(first), q, lay.first, rows, &any));
    HIP_TRY(ctx, octl_download(ctx, reinterpret_cast<uint32_t*>(size), q, lay.size, rows, &any));
    return OCTL_OK;
  };
  if (sure) OCTL_TRY(fetch((size_t)bound));
  HIP_TRY(ctx, hipMemcpyAsync(&total, rows_d, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&err, C.words + CL_W_ERR, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (err != 0) return cluster_budget_error(ctx, "cluster");
  if ((int64_t)total > bound)
    return octl_set_error(ctx, OCTL_E_STATE, "cluster: %lld rows for a bound of %lld", (long long)total,
                          (long long)bound);
  *n_rows = (int64_t)total;
  if (cap < (int64_t)total) return OCTL_OK;  // (a size query: nothing is written)
  if (!sure) {
    OCTL_TRY(fetch((size_t)total));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return OCTL_OK;
}

// octl_forest_remove_sparse step for step (radius.hip), with the components in the place of the counting self-query
int octl_forest_remove_small_clusters(octl_forest* f, double radius, int32_t min_points, const uint8_t* slot_sel,
                                      int32_t n_sel, int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  // (nearest_begin ends by making the index: what this entry refuses on its own comes first; before build
  //  nearest_begin itself refuses)
  if (f->built) {
    if (min_points < 1)
      return octl_set_error(ctx, OCTL_E_INVALID, "remove_small_clusters: min_points = %d is below 1", min_points);
    OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  }
  const bool some = f->n_ord > 0 && f->n_blocks > 0;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "remove_small_clusters", some ? 1 : 0, 1, radius, slot_sel, n_sel, true, &T));
  std::vector<uint32_t> off32;
  uint32_t* err_host = static_cast<uint32_t*>(ctx->small_host);  // (word 0 of the mirror: a target of small copies)
  if (some) {
    // (every buffer first: a failed allocation leaves the mask as it was)
    OCTL_TRY(mask_retire_reserve(f));
    BlockTable B;
    ClusterTables C;
    OCTL_TRY(cluster_components(f, T, radius, sel, off32, nullptr, &B, &C));
    {
      KTimer t(ctx, "cluster_mask");
      OCTL_LAUNCH(k_cluster_mask, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, ctx->stream, B, C, f->n_ord,
                  (uint32_t)min_points, f->mask_valid ? 0 : 1, f->mask.as<uint8_t>());
      HIP_TRY(ctx, hipGetLastError());
    }
    f->mask_valid = true;
    // (the error word travels in front of the compaction's counts: the one wait of mask_apply covers it)
    HIP_TRY(ctx, hipMemcpyAsync(err_host, C.words + CL_W_ERR, 4, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    OCTL_TRY(ensure_mask(f));
  }
  OCTL_TRY(mask_apply(f, n_alive));
  if (some && *err_host != 0) return cluster_budget_error(ctx, "remove_small_clusters");
  return OCTL_OK;
}

}  // extern "C"
