// How many stored points share the lattice cell of a point: octl_forest_cell_count, and the map-cleaning step made of
// it, octl_forest_thin - voxel-grid downsampling.  Defined by octreelib_amd/thinning.py:
// cell_count_np and thin_keep_np, and compared with them count for count.  No reference counterpart: the reference has
// no neighbour query.
//
//   the cell of p is floor(p / cell) per axis, the floor of the TRUE quotient (np.floor_divide) on an absolute lattice;
//   two points share a cell iff the three indices are equal.  Membership is decided without a division, on the sign
//   of two fused remainders (cell_walk.h: cell_holds) - this file is built with -ffp-contract=off like the rest, the
//   fma calls are explicit.
//
// Both kernels are the walk of cell_walk.h with a sink that counts:
//   k_cell_count  one query per lane, grid-stride, launched as k_radius_count is; one int32 per query;
//   k_thin_mask   the self-query: one wavefront per (leaf, pose) block of a tested pose, lanes striding over the
//                 block's positions of the ordered arrays (the mapping of k_sparse_mask); q = the stored bits of the
//                 position, rank = the stored points of its cell with a SMALLER store index, and mask[pos] = 0 where
//                 rank >= max_per_cell.  It reads xyz_ord, ord_idx and the tables and writes mask bytes of its own
//                 positions only, and never reads the mask: no order dependence, no atomics.
// No LDS, no scratch, no floating-point atomics; nothing is sized by the CU count except the grid of k_cell_count.
#include <algorithm>
#include <climits>
#include <cmath>

#include "cell_walk.h"
#include "common.h"
#include "forest.h"

namespace {

// every stored point of the cell counts, up to the cap
struct CellCount {
  int32_t n, cap;
  __host__ __device__ __forceinline__ void offer(uint32_t, uint32_t) { ++n; }
  __host__ __device__ __forceinline__ bool full() const { return n >= cap; }
};

// ... and only those before `self` in the order of the store (poses in slot order, rows in insertion order): the
// point itself never counts - the comparison is strict - and a duplicate at the same coordinates does when it is earlier
struct CellRank {
  int32_t n, cap;
  uint32_t self;
  __host__ __device__ __forceinline__ void offer(uint32_t idx, uint32_t) { n += idx < self ? 1 : 0; }
  __host__ __device__ __forceinline__ bool full() const { return n >= cap; }
};

__global__ __launch_bounds__(256) void k_cell_count(const double* __restrict__ xyz, int64_t n, double cell, int32_t cap,
                                                    NNTables T, int32_t* __restrict__ count_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    CellCount c = {0, cap};
    cell_walk(T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], cell, c);
    count_out[i] = c.n;
  }
}

// fill: no mask is pending, so every byte of every block is written here - 1 for what stays, the blocks of the poses
// that are not tested included; the blocks cover the ordered points exactly - instead of in a fill launch
// (k_sparse_mask does the same).  Otherwise only zeros are written, and a pending RANSAC mask stays in the bytes.
__global__ __launch_bounds__(256) void k_thin_mask(const uint32_t* __restrict__ blk_start,
                                                   const int32_t* __restrict__ blk_size,
                                                   const int32_t* __restrict__ blk_slot, int64_t nb,
                                                   const uint8_t* __restrict__ slot_sel, double cell,
                                                   int32_t max_per_cell, NNTables T, int fill,
                                                   uint8_t* __restrict__ mask) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  const bool tested = !slot_sel || slot_sel[blk_slot[b]] != 0;
  if (!tested && !fill) return;
  const int64_t n = blk_size[b], s0 = blk_start[b];
  for (int64_t i = threadIdx.x & 63; i < n; i += 64) {
    const int64_t pos = s0 + i;
    bool keep = true;
    if (tested) {
      const double* __restrict__ q = T.xyz_ord + 3 * pos;
      CellRank c = {0, max_per_cell, T.ord_idx[pos]};
      cell_walk(T, q[0], q[1], q[2], cell, c);
      keep = c.n < max_per_cell;
    }
    if (fill) mask[pos] = keep ? 1 : 0;
    else if (!keep) mask[pos] = 0;
  }
}

int launch_cell_count(octl_ctx* ctx, const double* xyz_dev, int64_t n, double cell, int32_t cap, const NNTables& T,
                      int32_t* count) {
  KTimer timer(ctx, "cell_count");
  const unsigned wgs = grid_stride_for(ctx, n);
  OCTL_LAUNCH(k_cell_count, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, cell, cap, T, count);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

// the refusals of both counting forms, then the tables and the index; *cap = the sink's cap
int cell_count_begin(octl_forest* f, int64_t n, double cell, int32_t max_count, const uint8_t* slot_sel, int32_t n_sel,
                     bool pointers_ok, NNTables* T, int32_t* cap) {
  // (cell_begin ends by making the index: what this entry refuses on its own comes first; before build cell_begin
  //  itself refuses)
  if (f->built && max_count < 0)
    return octl_set_error(f->ctx, OCTL_E_INVALID, "cell_count: max_count = %d is negative (0: uncapped)", max_count);
  OCTL_TRY(cell_begin(f, "cell_count", n, cell, slot_sel, n_sel, pointers_ok, T));
  *cap = max_count > 0 ? max_count : INT32_MAX;
  return OCTL_OK;
}

}  // namespace

// (the declaration: cell_walk.h)
int cell_begin(octl_forest* f, const char* what, int64_t n, double cell, const uint8_t* slot_sel, int32_t n_sel,
               bool pointers_ok, NNTables* T) {
  OCTL_TRY(query_begin(f, what, &T->t));
  octl_ctx* ctx = f->ctx;
  if (query_bad_count(n) || !pointers_ok) return octl_set_error(ctx, OCTL_E_INVALID, "bad %s arguments", what);
  if (!(std::isfinite(cell) && cell > 0.0))
    return octl_set_error(ctx, OCTL_E_INVALID, "%s: cell must be finite and positive", what);
  // every cell index of the map's domain stays below 2^50 in magnitude: indices and index + 1 are exact doubles.  A
  // grid's voxel indices are below 2^30, so L 2^-20 <= cell does it; cell <= L keeps a cell within two voxels per axis
  if (f->mode == 0 && cell > f->edge)
    return octl_set_error(ctx, OCTL_E_INVALID,
                          "%s: cell %g exceeds the voxel edge %g (a cell would touch more than 2 voxels per axis)",
                          what, cell, f->edge);
  if (f->mode == 0 && cell < f->edge * 0x1p-20)
    return octl_set_error(ctx, OCTL_E_INVALID, "%s: cell %g is below 2^-20 of the voxel edge %g", what, cell, f->edge);
  if (f->mode != 0) {
    double reach = 0.0;
    for (int a = 0; a < 3; ++a) reach = std::max(reach, std::max(std::fabs(f->corner[a]), std::fabs(f->corner[a] + f->edge)));
    if (!(reach / cell < CELL_INDEX_LIMIT))
      return octl_set_error(ctx, OCTL_E_INVALID, "%s: cell %g is below 2^-50 of the cube's reach %g", what, cell, reach);
  }
  return nn_tables(f, what, n, slot_sel, n_sel, T);
}

extern "C" {

int octl_forest_cell_count(octl_forest* f, const double* xyz, int64_t n, double cell, int32_t max_count,
                           const uint8_t* slot_sel, int32_t n_sel, int32_t* count) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  int32_t cap = 0;
  OCTL_TRY(cell_count_begin(f, n, cell, max_count, slot_sel, n_sel, n <= 0 || (xyz && count), &T, &cap));
  if (n == 0) return OCTL_OK;
  // host form: one upload, the kernel, one download, one wait
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  Carve plan;  // f->q_stage: [queries 3 f64 | count i32]
  const auto q_part = plan.add<double>((size_t)n * 3);
  const auto cnt_part = plan.add<int32_t>((size_t)n);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, plan.total));
  double* q_d = Carve::at(f->q_stage, q_part);
  int32_t* cnt_d = Carve::at(f->q_stage, cnt_part);
  HIP_TRY(ctx, hipMemcpyAsync(q_d, xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OCTL_TRY(launch_cell_count(ctx, q_d, n, cell, cap, T, cnt_d));
  HIP_TRY(ctx, hipMemcpyAsync(count, cnt_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_cell_count_device(octl_forest* f, const double* xyz_dev, int64_t n, double cell, int32_t max_count,
                                  const uint8_t* slot_sel, int32_t n_sel, int32_t* count_dev) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  int32_t cap = 0;
  OCTL_TRY(cell_count_begin(f, n, cell, max_count, slot_sel, n_sel, n <= 0 || (xyz_dev && count_dev), &T, &cap));
  if (n == 0) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return launch_cell_count(ctx, xyz_dev, n, cell, cap, T, count_dev);
}

// octl_forest_remove_sparse step for step (radius.hip), with the rank query in the place of the neighbour count
int octl_forest_thin(octl_forest* f, double cell, int32_t max_per_cell, const uint8_t* slot_sel, int32_t n_sel,
                     const uint8_t* among_sel, int32_t n_among, int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  // (cell_begin ends by making the index: what this entry refuses on its own comes first; before build cell_begin
  //  itself refuses)
  if (f->built) {
    if (max_per_cell < 1)
      return octl_set_error(ctx, OCTL_E_INVALID, "thin: max_per_cell = %d is below 1", max_per_cell);
    OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  }
  // (the walk is asked for one query when there is a point to judge: the index is made for `among`, and not at all
  //  for a map without ordered points)
  NNTables T;
  OCTL_TRY(cell_begin(f, "thin", f->n_ord > 0 && f->n_blocks > 0 ? 1 : 0, cell, among_sel, n_among, true, &T));
  hipStream_t st = ctx->stream;
  if (f->n_ord > 0 && f->n_blocks > 0) {
    // (every buffer first: a failed allocation leaves the mask as it was)
    OCTL_TRY(mask_retire_reserve(f));
    if (!sel.empty()) OCTL_TRY(devbuf_reserve(ctx, f->scheme_dev, sel.size()));
    if (!sel.empty()) {
      HIP_TRY(ctx, hipMemcpyAsync(f->scheme_dev.p, sel.data(), sel.size(), hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));  // (a pageable source)
    }
    KTimer t(ctx, "thin_mask");
    OCTL_LAUNCH(k_thin_mask, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st,
                (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                (const int32_t*)f->blk_slot.as<int32_t>(), f->n_blocks,
                sel.empty() ? (const uint8_t*)nullptr : (const uint8_t*)f->scheme_dev.as<uint8_t>(), cell,
                max_per_cell, T, f->mask_valid ? 0 : 1, f->mask.as<uint8_t>());
    HIP_TRY(ctx, hipGetLastError());
    f->mask_valid = true;
  } else {
    OCTL_TRY(ensure_mask(f));
  }
  return mask_apply(f, n_alive);
}

}  // extern "C"
