// The stored points nearest to a query point, within a radius: octl_forest_nearest.  Exact k-nearest
// search across leaf walls, defined by the brute force of octreelib_amd/query.py: nearest_np and compared with it
// bit for bit.  No reference counterpart: the reference has no neighbour query.
//
//   d2 = (dx dx + dy dy) + dz dz in f64, products and sums separate and in that order (-ffp-contract=off);
//   candidates d2 <= r2 = max_distance^2 (formed once on the host); order ascending (d2, slot, index in the pose).
//
// One kernel per call, one query per lane, grid-stride, no LDS, no scratch: the k best are a sorted list in registers
// (k is a template instance, compare-and-shift fully unrolled), the tree under a root is walked depth first WITHOUT a
// stack (parent / first_child; the child number of a node is node - first_child[parent[node]]), and a cube is skipped
// when a lower bound of the d2 of anything it can hold exceeds the k-th best so far.  The walk, cube_gap with the
// argument and the list are nearest_walk.h, shared with the matching kernel of the point registration.
// What a leaf holds comes from an index node -> run of (leaf, pose) blocks in slot order that is made once per forest
// state and pose selection (nn_prepare: the (node, slot) grouping of the selected blocks, leaf_moments.h: block_groups).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "leaf_moments.h"
#include "nearest_walk.h"
#include "query_walk.h"

namespace {

// One record and the run of every node from the sorted (node, slot) keys.  The head of a run counts it with a serial
// look ahead: the block table holds at most one block per (leaf, pose), so a run is at most n_poses keys long.  The
// record is written for every selected block, whatever its node; only a node inside the table gets a run.
__global__ __launch_bounds__(256) void k_nn_runs(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                 int64_t nb, int sbits, int kbits,
                                                 const uint32_t* __restrict__ blk_start,
                                                 const int32_t* __restrict__ blk_size,
                                                 const uint32_t* __restrict__ pose_off, int64_t n_nodes,
                                                 uint4* __restrict__ rec, int32_t* __restrict__ first,
                                                 int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const uint64_t k = key[i];
  if ((k >> kbits) != 0) return;  // (not selected: behind every selected block)
  const uint32_t b = val[i];
  const uint32_t slot = (uint32_t)(k & ((1ull << sbits) - 1));
  const uint64_t node = k >> sbits;
  rec[i] = make_uint4(blk_start[b], (uint32_t)blk_size[b], slot, pose_off[slot]);
  if (node >= (uint64_t)n_nodes) return;
  if (i == 0 || (key[i - 1] >> sbits) != node) {
    int32_t c = 1;
    while (i + c < nb && (key[i + c] >> kbits) == 0 && (key[i + c] >> sbits) == node) ++c;
    first[node] = (int32_t)i;
    cnt[node] = c;
  }
}

template <int KT>
__global__ __launch_bounds__(256) void k_nearest(const double* __restrict__ xyz, int64_t n, int k, double r, double r2,
                                                 NNTables T, int32_t* __restrict__ slot_out,
                                                 int64_t* __restrict__ index_out, double* __restrict__ d2_out,
                                                 int32_t* __restrict__ count_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double qx = xyz[3 * i + 0], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
    // the k best so far, ascending (d2, id), id = slot << 32 | index in the pose (nearest_walk.h: NNBest, the walk)
    // (the list is the kernel's own pair of arrays and the sink refers to them: with the arrays inside the sink the
    //  compiler keeps 175 VGPRs for k = 8 instead of 162 - DESIGN.md 4.19 has the table)
    double bd[KT];
    uint64_t bid[KT];
    NNBest<KT> best = {bd, bid};
    best.clear();
    nearest_walk(T, qx, qy, qz, r, r2, best);
    int32_t found = 0;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      if (j < k) {
        const bool has = bid[j] != ~0ull;
        found += has ? 1 : 0;
        slot_out[i * k + j] = has ? (int32_t)(bid[j] >> 32) : -1;
        index_out[i * k + j] = has ? (int64_t)(bid[j] & 0xffffffffull) : -1;
        d2_out[i * k + j] = bd[j];
      }
    }
    count_out[i] = found;
  }
}

template <int KT>
void launch_instance(octl_ctx* ctx, unsigned wgs, const double* xyz_dev, int64_t n, int k, double r, double r2,
                     const NNTables& T, int32_t* slot, int64_t* index, double* d2, int32_t* count) {
  OCTL_LAUNCH(k_nearest<KT>, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, k, r, r2, T, slot, index, d2, count);
}

int launch_nearest(octl_ctx* ctx, const double* xyz_dev, int64_t n, int k, double r, const NNTables& T, int32_t* slot,
                   int64_t* index, double* d2, int32_t* count) {
  KTimer timer(ctx, k <= 1 ? "nearest_k1" : k <= 2 ? "nearest_k2" : k <= 4 ? "nearest_k4" : "nearest_k8");
  const unsigned wgs = grid_stride_for(ctx, n);
  const double r2 = r * r;
  // (a request rounds up to the next instance and writes its first k columns)
  if (k <= 1) launch_instance<1>(ctx, wgs, xyz_dev, n, k, r, r2, T, slot, index, d2, count);
  else if (k <= 2) launch_instance<2>(ctx, wgs, xyz_dev, n, k, r, r2, T, slot, index, d2, count);
  else if (k <= 4) launch_instance<4>(ctx, wgs, xyz_dev, n, k, r, r2, T, slot, index, d2, count);
  else launch_instance<8>(ctx, wgs, xyz_dev, n, k, r, r2, T, slot, index, d2, count);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

}  // namespace

// (NNTab, the declaration: query_walk.h - raycast.hip reads the same index)
// the index node -> run of blocks for the selection `sel` (empty: every pose) of the forest as it stands
int nn_prepare(octl_forest* f, const std::vector<uint8_t>& sel) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const int64_t nb = f->n_blocks, n_nodes = f->nodes[f->cur].n;
  const int n_poses = (int)f->pose_off.size() - 1;
  f->nn_stamp = 0;
  const NNTab lay(nb, n_nodes);
  OCTL_TRY(devbuf_reserve(ctx, f->nn_tab, lay.plan.total));
  // (runs start empty: a node without a selected block, and every node of a forest without blocks, holds nothing)
  HIP_TRY(ctx, hipMemsetAsync(Carve::at(f->nn_tab, lay.first), 0, lay.plan.total - lay.first.off, st));
  if (nb > 0 && n_poses > 0) {
    // f->grp_scratch: the grouping (no rows), then [store offset u32 per pose]
    BlockGroups g(f, false);
    const auto off_part = g.plan.add<uint32_t>((size_t)n_poses);
    OCTL_TRY(g.prepare(f, sel));
    uint32_t* off_d = Carve::at(f->grp_scratch, off_part);
    std::vector<uint32_t> off32((size_t)n_poses);
    for (int s = 0; s < n_poses; ++s) off32[(size_t)s] = (uint32_t)f->pose_off[(size_t)s];  // (store indices are u32)
    HIP_TRY(ctx, hipMemcpyAsync(off_d, off32.data(), (size_t)n_poses * 4, hipMemcpyHostToDevice, st));
    {
      KTimer t(ctx, "nn_group");
      OCTL_TRY(block_groups(f, (int)sel.size(), nullptr, g));
      OCTL_LAUNCH(k_nn_runs, dim3(grid_for(nb)), dim3(256), 0, st, (const uint64_t*)g.keys[0],
                  (const uint32_t*)g.vals[0], nb, g.sbits, g.kbits, (const uint32_t*)f->blk_start.as<uint32_t>(),
                  (const int32_t*)f->blk_size.as<int32_t>(), (const uint32_t*)off_d, n_nodes,
                  Carve::at(f->nn_tab, lay.rec), Carve::at(f->nn_tab, lay.first), Carve::at(f->nn_tab, lay.cnt));
      HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (the uploads above read host arrays that end with this call)
  }
  f->nn_sel = sel;
  f->nn_stamp = f->content_stamp;
  return OCTL_OK;
}

// the tail of nearest_begin, shared with cell_begin (cell.hip): the selection, the refusal of displaced rows, then -
// for n > 0 - the index, made only when missing, stale or made for another selection, and the tables of the walk
// (T->t is the caller's, from query_begin).  The declaration: nearest_walk.h
int nn_tables(octl_forest* f, const char* what, int64_t n, const uint8_t* slot_sel, int32_t n_sel, NNTables* T) {
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  if (f->displaced_rows)
    return octl_set_error(ctx, OCTL_E_STATE,
                          "%s: map_leaf_points has moved rows outside their leaves - the search cannot bound "
                          "what a cube holds",
                          what);
  if (n == 0) return OCTL_OK;
  if (!(forest_table_valid(f, f->nn_stamp) && f->nn_sel == sel)) OCTL_TRY(nn_prepare(f, sel));
  const NodeTable& nt = f->nodes[f->cur];
  const NNTab lay(f->n_blocks, nt.n);
  T->parent = nt.parent.as<int32_t>();
  T->rec = Carve::at(f->nn_tab, lay.rec);
  T->first = Carve::at(f->nn_tab, lay.first);
  T->cnt = Carve::at(f->nn_tab, lay.cnt);
  T->xyz_ord = f->xyz_ord.as<double>();
  T->ord_idx = f->ord_idx.as<uint32_t>();
  T->max_steps = 4 * nt.n + 64;
  return OCTL_OK;
}

// what both forms start with, and octl_forest_point_registration_system (register_points.hip) too: the refusals, the
// tables, the index - made only when missing or stale (the declaration: nearest_walk.h)
int nearest_begin(octl_forest* f, const char* what, int64_t n, int32_t k, double max_distance, const uint8_t* slot_sel,
                  int32_t n_sel, bool pointers_ok, NNTables* T) {
  OCTL_TRY(query_begin(f, what, &T->t));
  octl_ctx* ctx = f->ctx;
  if (query_bad_count(n) || !pointers_ok) return octl_set_error(ctx, OCTL_E_INVALID, "bad %s arguments", what);
  if (k < 1 || k > OCTL_NN_MAX_K)
    return octl_set_error(ctx, OCTL_E_INVALID, "%s: k = %d is outside 1 .. %d", what, k, OCTL_NN_MAX_K);
  if (!(std::isfinite(max_distance) && max_distance > 0.0))
    return octl_set_error(ctx, OCTL_E_INVALID, "%s: max_distance must be finite and positive", what);
  if (f->mode == 0 && max_distance > 2.0 * f->edge)
    return octl_set_error(ctx, OCTL_E_INVALID,
                          "%s: max_distance %g exceeds twice the voxel edge %g (a query would touch more than 5 "
                          "voxels per axis)",
                          what, max_distance, f->edge);
  return nn_tables(f, what, n, slot_sel, n_sel, T);
}

extern "C" {

int octl_forest_nearest(octl_forest* f, const double* xyz, int64_t n, int32_t k, double max_distance,
                        const uint8_t* slot_sel, int32_t n_sel, int32_t* slot_out, int64_t* index_out, double* d2_out,
                        int32_t* count_out) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "nearest", n, k, max_distance, slot_sel, n_sel,
                         n <= 0 || (xyz && slot_out && index_out && d2_out && count_out), &T));
  if (n == 0) return OCTL_OK;
  // host form: one upload, the kernel, the downloads, one wait
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const size_t nk = (size_t)n * (size_t)k;
  Carve plan;  // f->q_stage: [queries 3 f64 | index i64 x k | d2 f64 x k | slot i32 x k | count i32]
  const auto q_part = plan.add<double>((size_t)n * 3);
  const auto idx_part = plan.add<int64_t>(nk);
  const auto d2_part = plan.add<double>(nk);
  const auto slot_part = plan.add<int32_t>(nk), cnt_part = plan.add<int32_t>((size_t)n);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, plan.total));
  double *q_d = Carve::at(f->q_stage, q_part), *d2_d = Carve::at(f->q_stage, d2_part);
  int64_t* idx_d = Carve::at(f->q_stage, idx_part);
  int32_t *slot_d = Carve::at(f->q_stage, slot_part), *cnt_d = Carve::at(f->q_stage, cnt_part);
  HIP_TRY(ctx, hipMemcpyAsync(q_d, xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OCTL_TRY(launch_nearest(ctx, q_d, n, k, max_distance, T, slot_d, idx_d, d2_d, cnt_d));
  HIP_TRY(ctx, hipMemcpyAsync(slot_out, slot_d, nk * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(index_out, idx_d, nk * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(d2_out, d2_d, nk * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(count_out, cnt_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_nearest_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t k, double max_distance,
                               const uint8_t* slot_sel, int32_t n_sel, int32_t* slot_dev, int64_t* index_dev,
                               double* d2_dev, int32_t* count_dev) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "nearest", n, k, max_distance, slot_sel, n_sel,
                         n <= 0 || (xyz_dev && slot_dev && index_dev && d2_dev && count_dev), &T));
  if (n == 0) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return launch_nearest(ctx, xyz_dev, n, k, max_distance, T, slot_dev, index_dev, d2_dev, count_dev);
}

}  // extern "C"
