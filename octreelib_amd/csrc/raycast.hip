// What does a ray hit first: octl_forest_raycast.  The first occupied leaf ("cube") or the first
// accepted pooled plane ("plane") along o + t d, t_min <= t <= t_max, defined by the brute force over the leaves of
// octreelib_amd/query.py: raycast_np and compared with it bit for bit.  No reference counterpart: the reference has
// no ray query.
//
//   per leaf (c, e), lo = c, hi = fl(c + e), per axis with inv = fl(1 / d):  a = fl(fl(lo - o) inv), b = fl(fl(hi - o) inv),
//   near = min(a, b), far = max(a, b); an axis with d == 0 or inv not finite passes iff lo <= o <= hi and bounds nothing;
//   t_in = max(nears, t_min), t_out = min(fars, t_max); crossed iff every such axis passes and t_in <= t_out.
//   cube:  candidates = crossed leaves with >= min_points alive points of the selected poses, t = t_in;
//   plane: candidates = crossed leaves whose pooled plane passes point_to_plane's gates, t = fl(num / den),
//          num = (nx fl(mx - ox) + ny fl(my - oy)) + nz fl(mz - oz), den = (nx dx + ny dy) + nz dz, den != 0, t_in <= t <= t_out;
//   answer = the candidate smallest in (t, node).  Every product, sum and quotient rounded (-ffp-contract=off).
//
// One kernel per call, one ray per lane, grid-stride, no LDS, no scratch.  Grid mode marches the slabs of voxels along
// the ray's major axis front to back and looks up the few voxels of a slab the ray can touch; under a root the tree is
// walked depth first without a stack (nearest.hip), children in front-to-back order.  A cube is skipped only by the
// SAME interval arithmetic on a box that contains every leaf below it (raycast_walk.h: ray_box has the argument), so no hit is lost.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "query_walk.h"
#include "raycast_walk.h"

namespace {

template <bool PLANE>
__global__ __launch_bounds__(256) void k_raycast(const double* __restrict__ org, const double* __restrict__ dir,
                                                 const double* __restrict__ t_min, const double* __restrict__ t_max,
                                                 int64_t n, RayTables T, int32_t* __restrict__ node_out,
                                                 double* __restrict__ t_out, int32_t* __restrict__ row_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const RayBest best = ray_cast<PLANE>(T, org + 3 * i, dir + 3 * i, t_min[i], t_max[i]);
    node_out[i] = best.node;
    t_out[i] = best.t;
    row_out[i] = best.row;
  }
}

template <bool PLANE>
int launch_raycast(octl_ctx* ctx, const double* org, const double* dir, const double* t_min, const double* t_max,
                   int64_t n, const RayTables& T, int32_t* node, double* t, int32_t* row) {
  KTimer timer(ctx, PLANE ? "raycast_plane" : "raycast_cube");
  const unsigned wgs = grid_stride_for(ctx, n);
  OCTL_LAUNCH(k_raycast<PLANE>, dim3(wgs), dim3(256), 0, ctx->stream, org, dir, t_min, t_max, n, T, node, t, row);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

// host form: a ray that is not dead must respect the grid's cap (a dead one is answered, not refused)
int raycast_check_cap(octl_forest* f, const double* t_min, const double* t_max, int64_t n) {
  if (f->mode != 0) return OCTL_OK;
  const double span = RAY_CAP_EDGES * f->edge, lim = RAY_T_LIMIT * f->edge;
  for (int64_t i = 0; i < n; ++i) {
    const double a = t_min[i], b = t_max[i];
    if (!(std::isfinite(a) && std::isfinite(b) && a <= b)) continue;
    if (!(b - a <= span))
      return octl_set_error(f->ctx, OCTL_E_INVALID,
                            "raycast: ray %lld spans t_max - t_min = %g, more than %g voxel edges of %g (the cap bounds a "
                            "call's cost)",
                            (long long)i, b - a, RAY_CAP_EDGES, f->edge);
    if (!(std::fabs(a) <= lim && std::fabs(b) <= lim))
      return octl_set_error(f->ctx, OCTL_E_INVALID, "raycast: ray %lld has |t| above 2^40 voxel edges of %g",
                            (long long)i, f->edge);
  }
  return OCTL_OK;
}

// what both forms start with: the refusals, the tables (made when missing, stale or made for another selection)
int raycast_begin(octl_forest* f, int64_t n, const uint8_t* slot_sel, int32_t n_sel, int32_t surface,
                  int32_t min_points, double max_variance, bool pointers_ok, const double* t_min_host,
                  const double* t_max_host, RayTables* T) {
  OCTL_TRY(query_begin(f, "raycast", &T->t));
  octl_ctx* ctx = f->ctx;
  if (query_bad_count(n) || !pointers_ok) return octl_set_error(ctx, OCTL_E_INVALID, "bad raycast arguments");
  if (surface != OCTL_RAY_CUBE && surface != OCTL_RAY_PLANE)
    return octl_set_error(ctx, OCTL_E_INVALID, "raycast: surface = %d is neither OCTL_RAY_CUBE nor OCTL_RAY_PLANE",
                          surface);
  if (min_points < 0) return octl_set_error(ctx, OCTL_E_INVALID, "raycast: min_points = %d is negative", min_points);
  if (std::isnan(max_variance)) return octl_set_error(ctx, OCTL_E_INVALID, "raycast: max_variance is NaN");
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  if (f->displaced_rows)
    return octl_set_error(ctx, OCTL_E_STATE,
                          "raycast: map_leaf_points has moved rows outside their leaves - a leaf's cube does not say "
                          "where its points are");
  if (n == 0) return OCTL_OK;
  if (t_min_host) OCTL_TRY(raycast_check_cap(f, t_min_host, t_max_host, n));
  const NodeTable& nt = f->nodes[f->cur];
  T->parent = nt.parent.as<int32_t>();
  T->first = T->cnt = nullptr;
  T->rec = nullptr;
  T->pt = PlaneTable{};
  T->min_points = min_points;
  T->max_steps = 4 * nt.n + 64;
  if (surface == OCTL_RAY_PLANE) {
    if (!(forest_table_valid(f, f->pl_stamp) && f->pl_sel == sel)) {
      f->seg_stamp = 0;  // (the segments were made from another table)
      OCTL_TRY(pooled_compute(f, sel));
    }
    OCTL_TRY(query_plane_table(f, "raycast", min_points, max_variance, &T->pt));
  } else {
    if (!(forest_table_valid(f, f->nn_stamp) && f->nn_sel == sel)) OCTL_TRY(nn_prepare(f, sel));
    const NNTab lay(f->n_blocks, nt.n);
    T->rec = Carve::at(f->nn_tab, lay.rec);
    T->first = Carve::at(f->nn_tab, lay.first);
    T->cnt = Carve::at(f->nn_tab, lay.cnt);
  }
  return OCTL_OK;
}

}  // namespace

extern "C" {

int octl_forest_raycast(octl_forest* f, const double* origins, const double* directions, const double* t_min,
                        const double* t_max, int64_t n, const uint8_t* slot_sel, int32_t n_sel, int32_t surface,
                        int32_t min_points, double max_variance, int32_t* node, double* t, int32_t* row) {
  if (!f) return OCTL_E_INVALID;
  RayTables T;
  OCTL_TRY(raycast_begin(f, n, slot_sel, n_sel, surface, min_points, max_variance,
                         n <= 0 || (origins && directions && t_min && t_max && node && t && row), t_min, t_max, &T));
  if (n == 0) return OCTL_OK;
  // one upload per input, the kernel, three downloads, one wait
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  Carve plan;  // f->q_stage: [origins 3 f64 | directions 3 f64 | t_min | t_max | t f64 | node i32 | row i32]
  const auto o_part = plan.add<double>((size_t)n * 3), d_part = plan.add<double>((size_t)n * 3);
  const auto a_part = plan.add<double>((size_t)n), b_part = plan.add<double>((size_t)n);
  const auto t_part = plan.add<double>((size_t)n);
  const auto node_part = plan.add<int32_t>((size_t)n), row_part = plan.add<int32_t>((size_t)n);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, plan.total));
  double *o_d = Carve::at(f->q_stage, o_part), *d_d = Carve::at(f->q_stage, d_part);
  double *a_d = Carve::at(f->q_stage, a_part), *b_d = Carve::at(f->q_stage, b_part);
  double* t_d = Carve::at(f->q_stage, t_part);
  int32_t *node_d = Carve::at(f->q_stage, node_part), *row_d = Carve::at(f->q_stage, row_part);
  HIP_TRY(ctx, hipMemcpyAsync(o_d, origins, (size_t)n * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_d, directions, (size_t)n * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(a_d, t_min, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(b_d, t_max, (size_t)n * 8, hipMemcpyHostToDevice, st));
  if (surface == OCTL_RAY_PLANE)
    OCTL_TRY(launch_raycast<true>(ctx, o_d, d_d, a_d, b_d, n, T, node_d, t_d, row_d));
  else
    OCTL_TRY(launch_raycast<false>(ctx, o_d, d_d, a_d, b_d, n, T, node_d, t_d, row_d));
  HIP_TRY(ctx, hipMemcpyAsync(node, node_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(t, t_d, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(row, row_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_raycast_device(octl_forest* f, const double* origins_dev, const double* directions_dev,
                               const double* t_min_dev, const double* t_max_dev, int64_t n, const uint8_t* slot_sel,
                               int32_t n_sel, int32_t surface, int32_t min_points, double max_variance,
                               int32_t* node_dev, double* t_dev, int32_t* row_dev) {
  if (!f) return OCTL_E_INVALID;
  RayTables T;
  OCTL_TRY(raycast_begin(f, n, slot_sel, n_sel, surface, min_points, max_variance,
                         n <= 0 || (origins_dev && directions_dev && t_min_dev && t_max_dev && node_dev && t_dev &&
                                    row_dev),
                         nullptr, nullptr, &T));
  if (n == 0) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  // (any of the inputs may be the target of an octl_dev_upload_async that is still in flight: ordered on the device)
  OCTL_TRY(ctx_wait_uploads(ctx, origins_dev, (size_t)n * 24));
  OCTL_TRY(ctx_wait_uploads(ctx, directions_dev, (size_t)n * 24));
  OCTL_TRY(ctx_wait_uploads(ctx, t_min_dev, (size_t)n * 8));
  OCTL_TRY(ctx_wait_uploads(ctx, t_max_dev, (size_t)n * 8));
  if (surface == OCTL_RAY_PLANE)
    return launch_raycast<true>(ctx, origins_dev, directions_dev, t_min_dev, t_max_dev, n, T, node_dev, t_dev, row_dev);
  return launch_raycast<false>(ctx, origins_dev, directions_dev, t_min_dev, t_max_dev, n, T, node_dev, t_dev, row_dev);
}

}  // extern "C"
