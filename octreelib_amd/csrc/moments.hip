// What the surface looks like round a point: count, mean, population covariance and its eigen-decomposition of the
// stored points within a radius of every query (octl_forest_neighbourhood_stats) and of every stored point
// (octl_forest_point_stats) - per-point normals, curvature and covariances.  Defined by
// octreelib_amd/neighbourhood.py: neighbourhood_statistics_np and point_statistics_np.  No reference counterpart: the
// reference has no neighbour query.
//
//   the neighbours of q are the candidates of octl_forest_radius_count, uncapped: the stored points p of the index with
//   d2 = (dx dx + dy dy) + dz dz <= r2 = radius^2, dx = q_x - p_x, in f64 with separate products and sums
//   (-ffp-contract=off) - the same walk (nearest_walk.h), the same cubes in the same order, the same d2 bits;
//   their moments are the shifted sums of leaf_moments.h about q, one point after the other in the order of the walk
//   (radius_moments.h: RadiusMoments), finished by finish() with p0 = q and decomposed by sym3_eigen.h.
//
//   k_neighbourhood_stats  one query per lane, grid-stride, launched as k_radius_count is;
//   k_point_stats          the self-query: one wavefront per (leaf, pose) block of a tested pose, lanes striding over
//                          the block's positions of the ordered arrays (the mapping of k_sparse_mask); q = the stored
//                          bits of the position, which counts itself when its pose is among the counted ones.  A wave
//                          books the rows of its block with one integer atomicAdd; every row carries the store index
//                          of its point, by which the host orders the rows - their place in the table means nothing.
// Both call moments_row (radius_moments.h) and nothing else, so a row's bits are a function of the tables and the
// query alone: the same from either kernel, in any batch.  No LDS, no scratch, no floating-point atomics.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "radius_moments.h"

namespace {

struct MomentRows {
  int64_t* count;  // [n]
  double* mean;    // [n][3]
  double* cov;     // [n][6]
  double* eigval;  // [n][3], nullptr: no decomposition
  double* eigvec;  // [n][9]
};

__device__ __forceinline__ void write_row(const NNTables& T, double qx, double qy, double qz, double r, double r2,
                                          const MomentRows& out, int64_t row) {
  out.count[row] = moments_row(T, qx, qy, qz, r, r2, out.mean + 3 * row, out.cov + 6 * row,
                               out.eigval ? out.eigval + 3 * row : nullptr, out.eigvec + 9 * row);
}

__global__ __launch_bounds__(256) void k_neighbourhood_stats(const double* __restrict__ xyz, int64_t n, double r,
                                                             double r2, NNTables T, MomentRows out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    write_row(T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], r, r2, out, i);
}

// cap: rows the table holds - the host's bound of the tested points; a block that would not fit writes nothing (and
// *n_rows then exceeds cap, which the host refuses)
__global__ __launch_bounds__(256) void k_point_stats(const uint32_t* __restrict__ blk_start,
                                                     const int32_t* __restrict__ blk_size,
                                                     const int32_t* __restrict__ blk_slot, int64_t nb,
                                                     const uint8_t* __restrict__ slot_sel, double r, double r2,
                                                     NNTables T, int64_t cap, unsigned long long* __restrict__ n_rows,
                                                     uint32_t* __restrict__ store_idx, MomentRows out) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  if (slot_sel && slot_sel[blk_slot[b]] == 0) return;
  const int64_t n = blk_size[b], s0 = blk_start[b];
  if (n <= 0) return;
  const int lane = threadIdx.x & 63;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(n_rows, (unsigned long long)n);
  base = __shfl(base, 0);
  if ((int64_t)base + n > cap) return;
  for (int64_t i = lane; i < n; i += 64) {
    const int64_t pos = s0 + i, row = (int64_t)base + i;
    const double* __restrict__ q = T.xyz_ord + 3 * pos;
    store_idx[row] = T.ord_idx[pos];
    write_row(T, q[0], q[1], q[2], r, r2, out, row);
  }
}

// f->q_stage of both forms: [queries 3 f64 | count i64 | mean | cov | eigval | eigvec | store index u32 | rows u64 |
// tested selection u8]; c rows, of which the host form brings its queries and the self-query its keys
struct MomentStage {
  size_t c, nq;
  Carve plan;
  Carve::Part<double> q = plan.add<double>(3 * nq);
  Carve::Part<int64_t> count = plan.add<int64_t>(c);
  Carve::Part<double> mean = plan.add<double>(3 * c), cov = plan.add<double>(6 * c), w = plan.add<double>(3 * c),
                      v = plan.add<double>(9 * c);
  Carve::Part<uint32_t> idx = plan.add<uint32_t>(nq ? 0 : c);
  Carve::Part<unsigned long long> rows = plan.add<unsigned long long>(1);
  Carve::Part<uint8_t> sel;
  MomentStage(int64_t rows_, bool queries, size_t n_sel)
      : c((size_t)std::max<int64_t>(rows_, 1)), nq(queries ? c : 0), sel(plan.add<uint8_t>(n_sel)) {}
  MomentRows table(DevBuf& b, bool eigen) {
    return MomentRows{Carve::at(b, count), Carve::at(b, mean), Carve::at(b, cov),
                      eigen ? Carve::at(b, w) : nullptr, Carve::at(b, v)};
  }
};

int launch_neighbourhood_stats(octl_ctx* ctx, const double* xyz_dev, int64_t n, double r, const NNTables& T,
                               const MomentRows& out) {
  KTimer timer(ctx, "neighbourhood_stats");
  const unsigned wgs = grid_stride_for(ctx, n);
  OCTL_LAUNCH(k_neighbourhood_stats, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, r, r * r, T, out);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

// the downloads of `rows` rows of a stage into the caller's arrays (any may be NULL)
int download_rows(octl_ctx* ctx, DevBuf& b, const MomentStage& lay, size_t rows, int64_t* count, double* mean,
                  double* cov, double* eigval, double* eigvec) {
  bool any = false;
  HIP_TRY(ctx, octl_download(ctx, count, b, lay.count, rows, &any));
  HIP_TRY(ctx, octl_download(ctx, mean, b, lay.mean, 3 * rows, &any));
  HIP_TRY(ctx, octl_download(ctx, cov, b, lay.cov, 6 * rows, &any));
  HIP_TRY(ctx, octl_download(ctx, eigval, b, lay.w, 3 * rows, &any));
  HIP_TRY(ctx, octl_download(ctx, eigvec, b, lay.v, 9 * rows, &any));
  return OCTL_OK;
}

}  // namespace

extern "C" {

int octl_forest_neighbourhood_stats(octl_forest* f, const double* xyz, int64_t n, double radius,
                                    const uint8_t* slot_sel, int32_t n_sel, int64_t* count, double* mean, double* cov,
                                    double* eigval, double* eigvec) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "neighbourhood_stats", n, 1, radius, slot_sel, n_sel,
                         n <= 0 || (xyz && (eigval != nullptr) == (eigvec != nullptr)), &T));
  if (n == 0) return OCTL_OK;
  // host form: one upload, the kernel, the downloads, one wait
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  MomentStage lay(n, true, 0);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, lay.plan.total));
  double* q_d = Carve::at(f->q_stage, lay.q);
  HIP_TRY(ctx, hipMemcpyAsync(q_d, xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OCTL_TRY(launch_neighbourhood_stats(ctx, q_d, n, radius, T, lay.table(f->q_stage, eigval != nullptr)));
  OCTL_TRY(download_rows(ctx, f->q_stage, lay, (size_t)n, count, mean, cov, eigval, eigvec));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_neighbourhood_stats_device(octl_forest* f, const double* xyz_dev, int64_t n, double radius,
                                           const uint8_t* slot_sel, int32_t n_sel, int64_t* count_dev,
                                           double* mean_dev, double* cov_dev, double* eigval_dev, double* eigvec_dev) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "neighbourhood_stats", n, 1, radius, slot_sel, n_sel,
                         n <= 0 || (xyz_dev && count_dev && mean_dev && cov_dev &&
                                    (eigval_dev != nullptr) == (eigvec_dev != nullptr)),
                         &T));
  if (n == 0) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return launch_neighbourhood_stats(ctx, xyz_dev, n, radius, T,
                                    MomentRows{count_dev, mean_dev, cov_dev, eigval_dev, eigvec_dev});
}

int octl_forest_point_stats(octl_forest* f, double radius, const uint8_t* slot_sel, int32_t n_sel,
                            const uint8_t* among_sel, int32_t n_among, int64_t cap, int64_t* n_rows, int32_t* slot,
                            int32_t* index, int64_t* count, double* mean, double* cov, double* eigval,
                            double* eigvec) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  if (f->built) {
    if (cap < 0 || !n_rows || (eigval != nullptr) != (eigvec != nullptr))
      return octl_set_error(ctx, OCTL_E_INVALID, "bad point_stats arguments");
    OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  }
  // (the walk is asked for one query when there is a point to describe: the index is made for `among`, and not at all
  //  for a map without ordered points)
  const bool some = f->n_ord > 0 && f->n_blocks > 0;
  NNTables T;
  OCTL_TRY(nearest_begin(f, "point_stats", some ? 1 : 0, 1, radius, among_sel, n_among, true, &T));
  *n_rows = 0;
  if (!some) return OCTL_OK;
  // the host's bound of the rows: the tested poses' rows of the store, and never more than the ordered points
  int64_t bound = 0;
  const size_t n_poses = f->pose_off.size() - 1;
  for (size_t s = 0; s < n_poses; ++s)
    if (sel.empty() || sel[s]) bound += f->pose_off[s + 1] - f->pose_off[s];
  bound = std::min(bound, f->n_ord);
  if (bound == 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  MomentStage lay(bound, false, sel.size());
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, lay.plan.total));
  unsigned long long* rows_d = Carve::at(f->q_stage, lay.rows);
  uint32_t* idx_d = Carve::at(f->q_stage, lay.idx);
  uint8_t* sel_d = sel.empty() ? nullptr : Carve::at(f->q_stage, lay.sel);
  HIP_TRY(ctx, hipMemsetAsync(rows_d, 0, 8, st));
  if (sel_d) HIP_TRY(ctx, hipMemcpyAsync(sel_d, sel.data(), sel.size(), hipMemcpyHostToDevice, st));
  {
    KTimer t(ctx, "point_stats");
    OCTL_LAUNCH(k_point_stats, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st,
                (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                (const int32_t*)f->blk_slot.as<int32_t>(), f->n_blocks, (const uint8_t*)sel_d, radius, radius * radius,
                T, bound, rows_d, idx_d, lay.table(f->q_stage, eigval != nullptr));
    HIP_TRY(ctx, hipGetLastError());
  }
  // one wait when the caller's arrays are known to hold every row (cap >= bound); otherwise the count first
  unsigned long long total = 0;
  const bool sure = cap >= bound;
  std::vector<uint32_t> idx;
  auto fetch = [&](size_t rows) -> int {
    idx.resize(rows);
    if (rows && (slot || index))
      HIP_TRY(ctx, hipMemcpyAsync(idx.data(), idx_d, rows * 4, hipMemcpyDeviceToHost, st));
    return download_rows(ctx, f->q_stage, lay, rows, count, mean, cov, eigval, eigvec);
  };
  if (sure) OCTL_TRY(fetch((size_t)bound));
  HIP_TRY(ctx, hipMemcpyAsync(&total, rows_d, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if ((int64_t)total > bound)
    return octl_set_error(ctx, OCTL_E_STATE, "point_stats: %lld rows for a bound of %lld", (long long)total,
                          (long long)bound);
  *n_rows = (int64_t)total;
  if (cap < (int64_t)total) return OCTL_OK;  // (a size query: nothing is written)
  if (!sure) {
    OCTL_TRY(fetch((size_t)total));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  // store index -> (slot, row of the pose's cloud as inserted)
  for (size_t i = 0; i < (size_t)total && (slot || index); ++i) {
    const int64_t g = idx[i];
    const size_t s = (size_t)(std::upper_bound(f->pose_off.begin(), f->pose_off.end(), g) - f->pose_off.begin()) - 1;
    if (slot) slot[i] = (int32_t)s;
    if (index) index[i] = (int32_t)(g - f->pose_off[s]);
  }
  return OCTL_OK;
}

}  // extern "C"
