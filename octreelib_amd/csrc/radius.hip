// How many stored points lie within a radius of a point: octl_forest_radius_count, and the map-cleaning step made of
// it, octl_forest_remove_sparse.  Defined by the brute force of octreelib_amd/query.py:
// radius_count_np and sparse_keep_np, and compared with them count for count.  No reference counterpart: the reference
// has no neighbour query.
//
//   d2 = (dx dx + dy dy) + dz dz in f64, products and sums separate and in that order (-ffp-contract=off);
//   a stored point counts iff d2 <= r2 = radius^2 (formed once on the host, inclusive): the candidates of nearest.
//
// Both kernels are the walk of octl_forest_nearest (nearest_walk.h: the same cubes in the same order, the same d2 bits)
// with a sink that counts instead of keeping a list:
//   k_radius_count  one query per lane, grid-stride, launched as k_nearest is; one int32 per query;
//   k_sparse_mask   the self-query: one wavefront per (leaf, pose) block of a tested pose, lanes striding over the
//                   block's positions of the ordered arrays (the mapping of k_carve_blocks - the lanes of a block share
//                   the leaf and with it nearly the whole walk); q = the stored bits of the position, the position
//                   itself excluded BY IDENTITY, and mask[pos] = 0 where fewer than min_neighbours others lie within
//                   the radius.  It reads xyz_ord and the tables and writes mask bytes of its own positions only: no
//                   order dependence, no atomics.
// No LDS, no scratch, no floating-point atomics; nothing is sized by the CU count except the grid of k_radius_count.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "nearest_walk.h"

namespace {

// The counting sink.  While the count is below the cap worst() is +inf: nothing prunes below r2, which is what a count
// needs.  Once the cap is reached it is negative: cur = fmin(r2, worst()) < 0 <= cube_bound for every cube and
// d2 <= cur for no point (d2 >= 0 or NaN), so the walk skips what is left and offers nothing more - sound because a
// saturated count cannot change.  self: the position of the ordered arrays that does not count (the self-query's own
// point); RADIUS_NO_SELF, which is no position (a forest holds fewer than 2^31 ordered points), for a plain query.
constexpr uint32_t RADIUS_NO_SELF = 0xffffffffu;
struct RadiusCount {
  int32_t n, cap;
  uint32_t self;
  __device__ __forceinline__ double worst() const {
    return n < cap ? __longlong_as_double(0x7ff0000000000000ll) : -1.0;
  }
  __device__ __forceinline__ void offer(double, uint64_t, uint32_t pos) { n += pos != self ? 1 : 0; }
};

__global__ __launch_bounds__(256) void k_radius_count(const double* __restrict__ xyz, int64_t n, double r, double r2,
                                                      int32_t cap, NNTables T, int32_t* __restrict__ count_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    RadiusCount c = {0, cap, RADIUS_NO_SELF};
    nearest_walk(T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], r, r2, c);
    count_out[i] = c.n;
  }
}

// fill: no mask is pending, so every byte of every block is written here - 1 for what stays, the blocks of the poses
// that are not tested included; the blocks cover the ordered points exactly - instead of in a fill launch
// (k_retire_mask does the same).  Otherwise only zeros are written, and a pending RANSAC mask stays in the bytes.
__global__ __launch_bounds__(256) void k_sparse_mask(const uint32_t* __restrict__ blk_start,
                                                     const int32_t* __restrict__ blk_size,
                                                     const int32_t* __restrict__ blk_slot, int64_t nb,
                                                     const uint8_t* __restrict__ slot_sel, double r, double r2,
                                                     int32_t min_neighbours, NNTables T, int fill,
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
      RadiusCount c = {0, min_neighbours, (uint32_t)pos};
      nearest_walk(T, q[0], q[1], q[2], r, r2, c);
      keep = c.n >= min_neighbours;
    }
    if (fill) mask[pos] = keep ? 1 : 0;
    else if (!keep) mask[pos] = 0;
  }
}

// the refusals of both counting forms, then the tables and the index (nearest_begin: made only when missing, stale or
// made for another selection); *cap = the sink's cap
int radius_count_begin(octl_forest* f, int64_t n, double radius, int32_t max_count, const uint8_t* slot_sel,
                       int32_t n_sel, bool pointers_ok, NNTables* T, int32_t* cap) {
  // (nearest_begin ends by making the index: what this entry refuses on its own comes first; before build
  //  nearest_begin itself refuses)
  if (f->built && max_count < 0)
    return octl_set_error(f->ctx, OCTL_E_INVALID, "radius_count: max_count = %d is negative (0: uncapped)", max_count);
  OCTL_TRY(nearest_begin(f, "radius_count", n, 1, radius, slot_sel, n_sel, pointers_ok, T));
  *cap = max_count > 0 ? max_count : INT32_MAX;
  return OCTL_OK;
}

int launch_radius_count(octl_ctx* ctx, const double* xyz_dev, int64_t n, double r, int32_t cap, const NNTables& T,
                        int32_t* count) {
  KTimer timer(ctx, "radius_count");
  const unsigned wgs = grid_stride_for(ctx, n);
  OCTL_LAUNCH(k_radius_count, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, r, r * r, cap, T, count);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

}  // namespace

extern "C" {

int octl_forest_radius_count(octl_forest* f, const double* xyz, int64_t n, double radius, int32_t max_count,
                             const uint8_t* slot_sel, int32_t n_sel, int32_t* count) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  int32_t cap = 0;
  OCTL_TRY(radius_count_begin(f, n, radius, max_count, slot_sel, n_sel, n <= 0 || (xyz && count), &T, &cap));
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
  OCTL_TRY(launch_radius_count(ctx, q_d, n, radius, cap, T, cnt_d));
  HIP_TRY(ctx, hipMemcpyAsync(count, cnt_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_radius_count_device(octl_forest* f, const double* xyz_dev, int64_t n, double radius, int32_t max_count,
                                    const uint8_t* slot_sel, int32_t n_sel, int32_t* count_dev) {
  if (!f) return OCTL_E_INVALID;
  NNTables T;
  int32_t cap = 0;
  OCTL_TRY(radius_count_begin(f, n, radius, max_count, slot_sel, n_sel, n <= 0 || (xyz_dev && count_dev), &T, &cap));
  if (n == 0) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return launch_radius_count(ctx, xyz_dev, n, radius, cap, T, count_dev);
}

// octl_forest_carve step for step (mask.hip: forest_carve), with the self-query in the place of k_carve_blocks
int octl_forest_remove_sparse(octl_forest* f, double radius, int32_t min_neighbours, const uint8_t* slot_sel,
                              int32_t n_sel, const uint8_t* among_sel, int32_t n_among, int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  // (nearest_begin ends by making the index: what this entry refuses on its own comes first; before build
  //  nearest_begin itself refuses)
  if (f->built) {
    if (min_neighbours < 1)
      return octl_set_error(ctx, OCTL_E_INVALID, "remove_sparse: min_neighbours = %d is below 1", min_neighbours);
    OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  }
  // (the walk is asked for one query when there is a point to judge: the index is made for `among`, and not at all
  //  for a map without ordered points)
  NNTables T;
  OCTL_TRY(nearest_begin(f, "remove_sparse", f->n_ord > 0 && f->n_blocks > 0 ? 1 : 0, 1, radius, among_sel, n_among,
                         true, &T));
  hipStream_t st = ctx->stream;
  if (f->n_ord > 0 && f->n_blocks > 0) {
    // (every buffer first: a failed allocation leaves the mask as it was)
    OCTL_TRY(mask_retire_reserve(f));
    if (!sel.empty()) OCTL_TRY(devbuf_reserve(ctx, f->scheme_dev, sel.size()));
    if (!sel.empty()) {
      HIP_TRY(ctx, hipMemcpyAsync(f->scheme_dev.p, sel.data(), sel.size(), hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));  // (a pageable source)
    }
    KTimer t(ctx, "sparse_mask");
    OCTL_LAUNCH(k_sparse_mask, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st,
                (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                (const int32_t*)f->blk_slot.as<int32_t>(), f->n_blocks,
                sel.empty() ? (const uint8_t*)nullptr : (const uint8_t*)f->scheme_dev.as<uint8_t>(), radius,
                radius * radius, min_neighbours, T, f->mask_valid ? 0 : 1, f->mask.as<uint8_t>());
    HIP_TRY(ctx, hipGetLastError());
    f->mask_valid = true;
  } else {
    OCTL_TRY(ensure_mask(f));
  }
  return mask_apply(f, n_alive);
}

}  // extern "C"
