// Per-(leaf, pose) point statistics on the device: count, mean, population covariance and its eigen-decomposition
// for a list of blocks of the forest's block table (octl_forest_leaf_stats).  The points are already leaf-ordered
// in xyz_ord and every block is one run [blk_start, blk_start + blk_size) of it, so the whole job is a segmented
// reduction plus one 3x3 eigensolve per block.
//
// The moments of a block with anchor p0 = its first point in storage order are
//   S = sum over the block's chunks c = 0, 1, ... (in that order) of P_c,
//   P_c = the 64-lane reduction of chunk c = points [c L, min((c+1) L, n)) of the block: lane l accumulates
//         d = p - p0 over the chunk's points l, l+64, ... (sums of d and of d d^T, f64, fma), then a butterfly
//         (xor 32, 16, ..., 1) that leaves the totals in every lane.
// mean = p0 + S_d / n, cov = S_dd / n - (S_d / n)(S_d / n)^T.  The shift is what makes the one-pass form safe:
// cancellation is relative to the block's extent, not to the magnitude of its coordinates.  S depends on the
// block's points and nothing else - not on where the block sits in the store, not on the other requested blocks -
// so a block's results are the same bits however it is requested.
//
// Launches (stream order, one host wait for the download):
//   [fill]          claim words of the block table + chunk counter (only when a block can exceed L points)
//   k_leaf_moments  one wave per requested block: a block of at most L points is reduced and finished here; a
//                   larger one is claimed by the first request that meets it, which books ceil(n / L) work items
//   k_leaf_chunks   [only when a block can exceed L points] one wave per work item (grid-stride): P_c of one chunk
//   k_leaf_eigen    one lane per requested block: folds the chunk partials of a large block in chunk order and
//                   finishes it, then the cyclic Jacobi of sym3_eigen.h
// A forest whose blocks are known to hold at most L points (a count-driven build with K <= L) skips the fill and
// k_leaf_chunks; should a larger block appear anyway, k_leaf_moments folds its chunks itself, in the same order and
// with the same arithmetic - the same bits, only slower.
#include <algorithm>

#include "common.h"
#include "forest.h"
#include "leaf_moments.h"
#include "sym3_eigen.h"

namespace {

__global__ __launch_bounds__(256) void k_leaf_moments(const int32_t* __restrict__ ids, int64_t nb,
                                                      const uint32_t* __restrict__ blk_start,
                                                      const int32_t* __restrict__ blk_size,
                                                      const double* __restrict__ xyz, int chunked,
                                                      int32_t* __restrict__ claim, uint32_t* __restrict__ counter,
                                                      int2* __restrict__ work, int64_t cap,
                                                      int64_t* __restrict__ count, double* __restrict__ mean,
                                                      double* __restrict__ cov) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nb) return;
  const int lane = threadIdx.x & 63;
  const int32_t b = ids[i];
  const int64_t s = blk_start[b];
  const int32_t n = blk_size[b];
  if (lane == 0) count[i] = n;
  if (n <= 0) {  // (the table holds non-empty blocks only)
    if (lane < 3) mean[3 * i + lane] = 0.0;
    if (lane < 6) cov[6 * i + lane] = 0.0;
    return;
  }
  if (chunked && n > LS_CHUNK) {
    // the first request of this block books its chunks; k_leaf_chunks reduces them, k_leaf_eigen folds them
    const int32_t nc = (n + LS_CHUNK - 1) / LS_CHUNK;
    int32_t off = -1;
    if (lane == 0 && atomicCAS(&claim[b], 0, -2) == 0) {
      const uint32_t o = atomicAdd(counter, (uint32_t)nc);
      const bool fits = (int64_t)o + nc <= cap;  // (always: the chunks of distinct blocks number < 2 n_ord / L)
      claim[b] = fits ? (int32_t)o + 1 : -1;
      off = fits ? (int32_t)o : -1;
    }
    off = __shfl(off, 0);
    if (off >= 0)
      for (int c = lane; c < nc; c += 64) work[off + c] = make_int2(b, c);
    return;
  }
  const double p0x = xyz[3 * s], p0y = xyz[3 * s + 1], p0z = xyz[3 * s + 2];
  Sums S = chunk_sums(xyz, s, min(n, LS_CHUNK), p0x, p0y, p0z, lane);
  for (int32_t c0 = LS_CHUNK; c0 < n; c0 += LS_CHUNK)  // (a large block on a forest without the chunk stage)
    fold(S, chunk_sums(xyz, s + c0, min(n - c0, LS_CHUNK), p0x, p0y, p0z, lane));
  if (lane == 0) finish(S, n, p0x, p0y, p0z, mean + 3 * i, cov + 6 * i);
}

__global__ __launch_bounds__(256) void k_leaf_chunks(const uint32_t* __restrict__ counter,
                                                     const int2* __restrict__ work, int64_t cap,
                                                     const uint32_t* __restrict__ blk_start,
                                                     const int32_t* __restrict__ blk_size,
                                                     const double* __restrict__ xyz, double* __restrict__ partial) {
  const int64_t total = min((int64_t)*counter, cap);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += waves) {
    const int2 w = work[t];
    const int64_t s = blk_start[w.x];
    const int32_t n = blk_size[w.x];
    const int32_t c0 = w.y * LS_CHUNK;
    const Sums P = chunk_sums(xyz, s + c0, min(n - c0, LS_CHUNK), xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2], lane);
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 9; ++k) partial[9 * t + k] = P.s[k];
  }
}

__global__ __launch_bounds__(256) void k_leaf_eigen(const int32_t* __restrict__ ids, int64_t nb,
                                                    const uint32_t* __restrict__ blk_start,
                                                    const int32_t* __restrict__ blk_size,
                                                    const double* __restrict__ xyz, int chunked,
                                                    const int32_t* __restrict__ claim, int64_t cap,
                                                    const double* __restrict__ partial, double* __restrict__ mean,
                                                    double* __restrict__ cov, double* __restrict__ eigval,
                                                    double* __restrict__ eigvec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  double c6[6];
  const int32_t b = ids[i];
  const int32_t n = blk_size[b];
  if (chunked && n > LS_CHUNK) {
    const int32_t nc = (n + LS_CHUNK - 1) / LS_CHUNK;
    const int64_t base = (int64_t)claim[b] - 1;
    const int64_t s = blk_start[b];
    double m3[3];
    if (base >= 0 && base + nc <= cap) {
      Sums S;
#pragma unroll
      for (int k = 0; k < 9; ++k) S.s[k] = partial[9 * base + k];
      for (int32_t c = 1; c < nc; ++c) {
        Sums P;
#pragma unroll
        for (int k = 0; k < 9; ++k) P.s[k] = partial[9 * (base + c) + k];
        fold(S, P);
      }
      finish(S, n, xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2], m3, c6);
    } else {  // (unreachable: the work list is sized for every chunk)
      const double q = __longlong_as_double(0x7ff8000000000000ll);
      m3[0] = m3[1] = m3[2] = q;
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = q;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[3 * i + k] = m3[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) cov[6 * i + k] = c6[k];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov[6 * i + k];
  }
  if (!eigval) return;
  double w[3], v[9];
  sym3_eigen(c6, w, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) eigval[3 * i + k] = w[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) eigvec[9 * i + k] = v[k];
}

__global__ __launch_bounds__(256) void k_sym3_eigen(const double* __restrict__ c6, int64_t n,
                                                    double* __restrict__ eigval, double* __restrict__ eigvec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double c[6], w[3], v[9];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = c6[6 * i + k];
  sym3_eigen(c, w, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) eigval[3 * i + k] = w[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) eigvec[9 * i + k] = v[k];
}

}  // namespace

extern "C" int octl_forest_leaf_stats(octl_forest* f, const int32_t* block_ids, int64_t nb, int64_t* count,
                                      double* mean, double* cov, double* eigval, double* eigvec) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "leaf_stats before build");
  if (nb < 0 || (nb > 0 && !block_ids)) return octl_set_error(ctx, OCTL_E_INVALID, "bad leaf_stats arguments");
  if (nb >= ((int64_t)1 << 31)) return octl_set_error(ctx, OCTL_E_INVALID, "too many blocks in one leaf_stats call");
  for (int64_t i = 0; i < nb; ++i)
    if (block_ids[i] < 0 || block_ids[i] >= f->n_blocks)
      return octl_set_error(ctx, OCTL_E_INVALID, "block index %lld out of range [0, %lld)", (long long)block_ids[i],
                            (long long)f->n_blocks);
  if (nb == 0) return OCTL_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool eigen = eigval || eigvec;
  const bool chunked = f->max_block_hint > LS_CHUNK;
  // at most ceil(n / L) < 2 n / L chunks per block of n > L points, and the blocks are disjoint runs of xyz_ord
  const int64_t cap = chunked ? 2 * f->n_ord / LS_CHUNK + 2 : 0;
  // ctx->ls_buf: [ids i32 | count i64 | mean 3 f64 | cov 6 f64 | eigval 3 f64 | eigvec 9 f64 | counter (16 bytes) +
  //               claim i32 per table block | work items int2 | chunk partials 9 f64]
  Carve plan;
  const size_t n = (size_t)nb, ne = eigen ? n : 0, claim_bytes = chunked ? 16 + (size_t)f->n_blocks * 4 : 0;
  const auto ids_p = plan.add<int32_t>(n);
  const auto cnt_p = plan.add<int64_t>(n);
  const auto mean_p = plan.add<double>(3 * n), cov_p = plan.add<double>(6 * n);
  const auto w_p = plan.add<double>(3 * ne), v_p = plan.add<double>(9 * ne);
  const auto counter_p = plan.add<uint32_t>(claim_bytes / 4);
  const auto work_p = plan.add<int2>((size_t)cap);
  const auto part_p = plan.add<double>(9 * (size_t)cap);
  OCTL_TRY(devbuf_reserve(ctx, ctx->ls_buf, plan.total));
  DevBuf& lb = ctx->ls_buf;
  int32_t* ids_d = Carve::at(lb, ids_p);
  int64_t* cnt_d = Carve::at(lb, cnt_p);
  double *mean_d = Carve::at(lb, mean_p), *cov_d = Carve::at(lb, cov_p), *part_d = Carve::at(lb, part_p);
  double *w_d = eigen ? Carve::at(lb, w_p) : nullptr, *v_d = eigen ? Carve::at(lb, v_p) : nullptr;
  uint32_t* counter_d = Carve::at(lb, counter_p);
  int32_t* claim_d = reinterpret_cast<int32_t*>(counter_d + 4);
  int2* work_d = Carve::at(lb, work_p);
  const uint32_t* bstart = f->blk_start.as<uint32_t>();
  const int32_t* bsize = f->blk_size.as<int32_t>();
  const double* xyz = f->xyz_ord.as<double>();

  HIP_TRY(ctx, hipMemcpyAsync(ids_d, block_ids, (size_t)nb * 4, hipMemcpyHostToDevice, st));
  if (chunked) HIP_TRY(ctx, hipMemsetAsync(counter_d, 0, claim_bytes, st));
  {
    KTimer t(ctx, "leaf_moments");
    OCTL_LAUNCH(k_leaf_moments, dim3((unsigned)ceil_div(nb, 4)), dim3(256), 0, st, (const int32_t*)ids_d, nb, bstart,
                bsize, xyz, (int)chunked, claim_d, counter_d, work_d, cap, cnt_d, mean_d, cov_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (chunked) {
    KTimer t(ctx, "leaf_chunks");
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(ceil_div(cap, 4), (int64_t)octl_ctx_cus(ctx) * 8));
    OCTL_LAUNCH(k_leaf_chunks, dim3((unsigned)wgs), dim3(256), 0, st, (const uint32_t*)counter_d,
                (const int2*)work_d, cap, bstart, bsize, xyz, part_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (chunked || eigen) {
    KTimer t(ctx, "leaf_eigen");
    OCTL_LAUNCH(k_leaf_eigen, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, (const int32_t*)ids_d, nb, bstart,
                bsize, xyz, (int)chunked, (const int32_t*)claim_d, cap, (const double*)part_d, mean_d, cov_d, w_d,
                v_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (count) HIP_TRY(ctx, hipMemcpyAsync(count, cnt_d, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
  if (mean) HIP_TRY(ctx, hipMemcpyAsync(mean, mean_d, (size_t)nb * 24, hipMemcpyDeviceToHost, st));
  if (cov) HIP_TRY(ctx, hipMemcpyAsync(cov, cov_d, (size_t)nb * 48, hipMemcpyDeviceToHost, st));
  if (eigval) HIP_TRY(ctx, hipMemcpyAsync(eigval, w_d, (size_t)nb * 24, hipMemcpyDeviceToHost, st));
  if (eigvec) HIP_TRY(ctx, hipMemcpyAsync(eigvec, v_d, (size_t)nb * 72, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

extern "C" int octl_debug_sym3_eigen(octl_ctx* ctx, const double* cov6, int64_t n, double* eigval, double* eigvec) {
  if (!ctx) return OCTL_E_INVALID;
  if (n < 0 || (n > 0 && (!cov6 || !eigval || !eigvec)))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad sym3_eigen arguments");
  if (n == 0) return OCTL_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Carve plan;
  const auto c_p = plan.add<double>(6 * (size_t)n), w_p = plan.add<double>(3 * (size_t)n);
  const auto v_p = plan.add<double>(9 * (size_t)n);
  OCTL_TRY(devbuf_reserve(ctx, ctx->ls_buf, plan.total));
  double *c_d = Carve::at(ctx->ls_buf, c_p), *w_d = Carve::at(ctx->ls_buf, w_p), *v_d = Carve::at(ctx->ls_buf, v_p);
  HIP_TRY(ctx, hipMemcpyAsync(c_d, cov6, (size_t)n * 48, hipMemcpyHostToDevice, st));
  OCTL_LAUNCH(k_sym3_eigen, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, (const double*)c_d, n, w_d, v_d);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(eigval, w_d, (size_t)n * 24, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(eigvec, v_d, (size_t)n * 72, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

// ---- pooled planes: one plane per leaf over a selection of poses (octl_forest_pooled_leaf_stats) ----------------------
// A map plane pools the poses that observed the leaf.  The (leaf, pose) blocks of the selected poses are grouped by
// leaf on the device - sort of (node << slot bits | slot, block id), head flags, exclusive scan: row r = the r-th
// leaf in ascending node id - and every leaf is reduced by one wave:
//   anchor a = the leaf's centre, corner + edge / 2 (what split_planar.hip shifts by: the points of a leaf lie within
//   edge / 2 of it unless map_leaf_points moved them),
//   S = the leaf's blocks in ascending slot order, each block the sum over its chunks c = 0, 1, ... of P_c
//       (chunk_sums above, d = p - a), the first block's sums taken as they are and every later one added to them,
//   mean = a + S_d / n, cov = S_dd / n - (S_d / n)(S_d / n)^T (finish above), then sym3_eigen per row.
// A leaf's bits depend on its own points and on the selection only.  The table stays on the device (forest.h) for
// octl_forest_point_to_plane.
namespace {

// one wave per sorted position; the wave of a leaf's first block reduces the whole leaf
__global__ __launch_bounds__(256) void k_pool_moments(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                      const uint32_t* __restrict__ row_of, int64_t nb, int sbits,
                                                      int kbits, const uint32_t* __restrict__ blk_start,
                                                      const int32_t* __restrict__ blk_size,
                                                      const double* __restrict__ xyz,
                                                      const double* __restrict__ corner,
                                                      const double* __restrict__ edge, int64_t n_rows,
                                                      int32_t* __restrict__ node_out, int64_t* __restrict__ count,
                                                      double* __restrict__ mean, double* __restrict__ cov) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nb) return;
  const int lane = threadIdx.x & 63;
  const uint64_t k = key[i];
  if ((k >> kbits) != 0) return;
  const uint64_t node = k >> sbits;
  if (i > 0 && (key[i - 1] >> sbits) == node) return;
  const int64_t row = row_of[i];
  if (row >= n_rows) return;  // (never: the tables are sized from the scan's total)
  const double h = edge[node] / 2.0;
  const double ax = corner[3 * node + 0] + h, ay = corner[3 * node + 1] + h, az = corner[3 * node + 2] + h;
  Sums S;
#pragma unroll
  for (int q = 0; q < 9; ++q) S.s[q] = 0.0;
  int64_t n_all = 0;
  for (int64_t j = i; j < nb && (key[j] >> sbits) == node; ++j) {
    const uint32_t b = val[j];
    const int64_t s = blk_start[b];
    const int32_t n = blk_size[b];
    Sums B = chunk_sums(xyz, s, min(n, LS_CHUNK), ax, ay, az, lane);
    for (int32_t c0 = LS_CHUNK; c0 < n; c0 += LS_CHUNK)
      fold(B, chunk_sums(xyz, s + c0, min(n - c0, LS_CHUNK), ax, ay, az, lane));
    if (j == i) S = B; else fold(S, B);
    n_all += n;
  }
  if (lane == 0) {
    node_out[row] = (int32_t)node;
    count[row] = n_all;
    finish(S, n_all, ax, ay, az, mean + 3 * row, cov + 6 * row);
  }
}

// one lane per row: eigen-decomposition, the 64-byte plane row of octl_forest_point_to_plane, node -> row
__global__ __launch_bounds__(256) void k_pool_eigen(int64_t n_rows, const int32_t* __restrict__ node,
                                                    const int64_t* __restrict__ count, const double* __restrict__ mean,
                                                    const double* __restrict__ cov, double* __restrict__ eigval,
                                                    double* __restrict__ eigvec, double* __restrict__ plane,
                                                    int32_t* __restrict__ node_row) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  double c6[6], w[3], v[9];
#pragma unroll
  for (int k = 0; k < 6; ++k) c6[k] = cov[6 * r + k];
  sym3_eigen(c6, w, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) eigval[3 * r + k] = w[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) eigvec[9 * r + k] = v[k];
  double* p = plane + 8 * r;
  p[0] = v[0], p[1] = v[3], p[2] = v[6];
  p[3] = mean[3 * r + 0], p[4] = mean[3 * r + 1], p[5] = mean[3 * r + 2];
  p[6] = w[0];
  p[7] = (double)count[r];
  node_row[node[r]] = (int32_t)r;
}

}  // namespace

// (PoolLayout: forest.h)
int pooled_compute(octl_forest* f, const std::vector<uint8_t>& sel) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const int64_t nb = f->n_blocks, n_nodes = f->nodes[f->cur].n;
  f->pl_stamp = 0;
  OCTL_TRY(devbuf_reserve(ctx, f->pl_node_row, (size_t)std::max<int64_t>(n_nodes, 1) * 4));
  if (n_nodes > 0) HIP_TRY(ctx, hipMemsetAsync(f->pl_node_row.p, 0xFF, (size_t)n_nodes * 4, st));
  int64_t n_rows = 0;
  if (nb > 0) {
    BlockGroups g(f, true);
    const auto total_part = g.plan.add<uint32_t>(1);
    OCTL_TRY(g.prepare(f, sel));
    uint32_t* total_d = Carve::at(f->grp_scratch, total_part);
    {
      KTimer t(ctx, "pool_group");
      OCTL_TRY(block_groups(f, (int)sel.size(), total_d, g));
    }
    uint32_t total = 0;
    OCTL_TRY(octl_readback(ctx, total_d, 1, &total));
    n_rows = total;
    if (n_rows > 0) {
      const PoolLayout lay(n_rows);
      OCTL_TRY(devbuf_reserve(ctx, f->pl_rows, lay.plan.total));
      OCTL_TRY(devbuf_reserve(ctx, f->pl_plane, (size_t)n_rows * 64));
      int32_t* node_d = Carve::at(f->pl_rows, lay.node);
      int64_t* cnt_d = Carve::at(f->pl_rows, lay.count);
      double *mean_d = Carve::at(f->pl_rows, lay.mean), *cov_d = Carve::at(f->pl_rows, lay.cov);
      {
        KTimer t(ctx, "pool_moments");
        const NodeTable& nt = f->nodes[f->cur];
        OCTL_LAUNCH(k_pool_moments, dim3((unsigned)ceil_div(nb, 4)), dim3(256), 0, st, (const uint64_t*)g.keys[0],
                    (const uint32_t*)g.vals[0], (const uint32_t*)g.heads, nb, g.sbits, g.kbits,
                    (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                    (const double*)f->xyz_ord.as<double>(), (const double*)nt.corner.as<double>(),
                    (const double*)nt.edge.as<double>(), n_rows, node_d, cnt_d, mean_d, cov_d);
        HIP_TRY(ctx, hipGetLastError());
      }
      {
        KTimer t(ctx, "pool_eigen");
        OCTL_LAUNCH(k_pool_eigen, dim3(grid_for(n_rows)), dim3(256), 0, st, n_rows, (const int32_t*)node_d,
                    (const int64_t*)cnt_d, (const double*)mean_d, (const double*)cov_d,
                    Carve::at(f->pl_rows, lay.w), Carve::at(f->pl_rows, lay.v), f->pl_plane.as<double>(),
                    f->pl_node_row.as<int32_t>());
        HIP_TRY(ctx, hipGetLastError());
      }
    }
  }
  f->pl_n = f->pl_cap = n_rows;
  f->pl_sel = sel;
  f->pl_stamp = f->content_stamp;
  return OCTL_OK;
}

extern "C" int octl_forest_pooled_leaf_stats(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int64_t cap,
                                             int32_t* node, int64_t* count, double* mean, double* cov6, double* eigval,
                                             double* eigvec, int64_t* n_leaves) {
  if (!f || !n_leaves) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "pooled_leaf_stats before build");
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (a fill behind a size query finds the table the query made: the same selection on an unchanged forest)
  if (!(forest_table_valid(f, f->pl_stamp) && f->pl_sel == sel)) OCTL_TRY(pooled_compute(f, sel));
  *n_leaves = f->pl_n;
  const int64_t n = f->pl_n;
  if (n <= 0 || cap < n) return OCTL_OK;
  const PoolLayout lay(f->pl_cap);
  bool any = false;
  HIP_TRY(ctx, octl_download(ctx, node, f->pl_rows, lay.node, (size_t)n, &any));
  HIP_TRY(ctx, octl_download(ctx, count, f->pl_rows, lay.count, (size_t)n, &any));
  HIP_TRY(ctx, octl_download(ctx, mean, f->pl_rows, lay.mean, (size_t)n * 3, &any));
  HIP_TRY(ctx, octl_download(ctx, cov6, f->pl_rows, lay.cov, (size_t)n * 6, &any));
  HIP_TRY(ctx, octl_download(ctx, eigval, f->pl_rows, lay.w, (size_t)n * 3, &any));
  HIP_TRY(ctx, octl_download(ctx, eigvec, f->pl_rows, lay.v, (size_t)n * 9, &any));
  if (any) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OCTL_OK;
}
