// Read-only queries against the scheme: which leaf does a point fall into (octl_forest_locate), and how far is it
// from that leaf's pooled least-squares plane (octl_forest_point_to_plane; the planes are those of the last
// octl_forest_pooled_leaf_stats, leaf_stats.hip).  No reference counterpart: the reference answers such a question
// by inserting the points (octree/octree.py:67-100), which changes the tree.
//
// A query is placed exactly as the point of a late pose is (incremental.hip: k_inc_place) because both run the same
// walk (scheme_walk.h); where the insertion would raise, count a new voxel or hand over to the general path, the
// query answers -1 and touches nothing - not the tables, not the context's error word.
//
// One kernel per call, grid-stride, one query per lane, no LDS.  The walk keeps the chain of dependent loads of the
// insertion (first_child -> corner, edge per level) instead of carrying the cube down from the root: the node table
// of a 10 M point scene is a few tens of MB (L2 and Infinity Cache hold it), and identity with k_inc_place is then a
// property of the shared code rather than of an argument about dyadic cubes (DESIGN.md 4.8 has the measurement).
// point_to_plane fuses the lookup into the same kernel: the point is in registers, the plane is one 64-byte row
// {normal, mean, lambda0, count} = four aligned 16-byte loads from one cache line.
#include <algorithm>

#include "common.h"
#include "forest.h"
#include "query_walk.h"

namespace {

template <bool PLANE>
__global__ __launch_bounds__(256) void k_query(const double* __restrict__ xyz, int64_t n, QueryTables t, PlaneTable pt,
                                               int32_t* __restrict__ node_out, int32_t* __restrict__ row_out,
                                               double* __restrict__ dist_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double px = xyz[3 * i + 0], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const int32_t node = locate_one(t, px, py, pz);
    node_out[i] = node;
    if (PLANE) {
      int32_t row;
      double nrm[3];
      const double d = plane_residual(pt, node, px, py, pz, &row, nrm);
      row_out[i] = row;
      dist_out[i] = d;
    }
  }
}

template <bool PLANE>
int launch_query(octl_ctx* ctx, const char* name, const double* xyz_dev, int64_t n, const QueryTables& t,
                 const PlaneTable& pt, int32_t* node, int32_t* row, double* dist) {
  KTimer timer(ctx, name);
  OCTL_LAUNCH(k_query<PLANE>, dim3(grid_stride_for(ctx, n)), dim3(256), 0, ctx->stream, xyz_dev, n, t, pt, node, row, dist);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

// host form: one upload, the kernel, the downloads, one wait
template <bool PLANE>
int query_host(octl_forest* f, const char* name, const double* xyz, int64_t n, const QueryTables& t,
               const PlaneTable& pt, int32_t* node, int32_t* row, double* dist) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const size_t o_node = align256((size_t)n * 24), o_row = o_node + align256((size_t)n * 4);
  const size_t o_dist = o_row + (PLANE ? align256((size_t)n * 4) : 0);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, o_dist + (PLANE ? (size_t)n * 8 : 0)));
  char* base = static_cast<char*>(f->q_stage.p);
  int32_t* node_d = reinterpret_cast<int32_t*>(base + o_node);
  int32_t* row_d = reinterpret_cast<int32_t*>(base + o_row);
  double* dist_d = reinterpret_cast<double*>(base + o_dist);
  HIP_TRY(ctx, hipMemcpyAsync(base, xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OCTL_TRY(launch_query<PLANE>(ctx, name, reinterpret_cast<const double*>(base), n, t, pt, node_d, row_d, dist_d));
  HIP_TRY(ctx, hipMemcpyAsync(node, node_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (PLANE) {
    HIP_TRY(ctx, hipMemcpyAsync(row, row_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(dist, dist_d, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

}  // namespace

// (query_walk.h: shared with register.hip)
int query_begin(octl_forest* f, const char* what, QueryTables* t) {
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "%s before build", what);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  OCTL_TRY(forest_sync_vcodes(f));
  const NodeTable& nt = f->nodes[f->cur];
  t->mode = f->mode;
  t->L = f->edge;
  t->org = f->vorg;
  t->vcode = f->vcode_dev[0].as<uint64_t>();
  t->V = f->n_voxels;
  t->first_child = nt.first_child.as<int32_t>();
  t->corner = nt.corner.as<double>();
  t->edge = nt.edge.as<double>();
  return OCTL_OK;
}

int query_plane_table(octl_forest* f, const char* what, int32_t min_points, double max_variance, PlaneTable* pt) {
  octl_ctx* ctx = f->ctx;
  if (!forest_table_valid(f, f->pl_stamp)) {
    if (!f->pl_node_row.p)
      return octl_set_error(ctx, OCTL_E_STATE,
                            "%s: the forest has no pooled leaf planes (call octl_forest_pooled_leaf_stats first)",
                            what);
    return octl_set_error(ctx, OCTL_E_STATE,
                          "%s: the pooled leaf planes are stale - the forest's contents or scheme changed after "
                          "octl_forest_pooled_leaf_stats made them",
                          what);
  }
  pt->node_row = f->pl_node_row.as<int32_t>();
  pt->rows = f->pl_plane.as<double2>();
  pt->min_points = min_points;
  pt->max_variance = max_variance >= 0.0 ? max_variance : -1.0;
  return OCTL_OK;
}

extern "C" {

int octl_forest_locate(octl_forest* f, const double* xyz, int64_t n, int32_t* node) {
  if (!f) return OCTL_E_INVALID;
  QueryTables t;
  OCTL_TRY(query_begin(f, "locate", &t));
  if (query_bad_count(n) || (n > 0 && (!xyz || !node)))
    return octl_set_error(f->ctx, OCTL_E_INVALID, "bad locate arguments");
  if (n == 0) return OCTL_OK;
  return query_host<false>(f, "locate", xyz, n, t, PlaneTable{}, node, nullptr, nullptr);
}

int octl_forest_locate_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t* node_dev) {
  if (!f) return OCTL_E_INVALID;
  QueryTables t;
  OCTL_TRY(query_begin(f, "locate", &t));
  octl_ctx* ctx = f->ctx;
  if (query_bad_count(n) || (n > 0 && (!xyz_dev || !node_dev)))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad locate arguments");
  if (n == 0) return OCTL_OK;
  // (the points may be the target of an octl_dev_upload_async that is still in flight: ordered on the device)
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return launch_query<false>(ctx, "locate", xyz_dev, n, t, PlaneTable{}, node_dev, nullptr, nullptr);
}

int octl_forest_point_to_plane(octl_forest* f, const double* xyz, int64_t n, int32_t min_points, double max_variance,
                               int32_t* node, int32_t* row, double* distance) {
  if (!f) return OCTL_E_INVALID;
  QueryTables t;
  OCTL_TRY(query_begin(f, "point_to_plane", &t));
  PlaneTable pt;
  OCTL_TRY(query_plane_table(f, "point_to_plane", min_points, max_variance, &pt));
  if (query_bad_count(n) || (n > 0 && (!xyz || !node || !row || !distance)))
    return octl_set_error(f->ctx, OCTL_E_INVALID, "bad point_to_plane arguments");
  if (n == 0) return OCTL_OK;
  return query_host<true>(f, "point_to_plane", xyz, n, t, pt, node, row, distance);
}

int octl_forest_point_to_plane_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t min_points,
                                      double max_variance, int32_t* node_dev, int32_t* row_dev,
                                      double* distance_dev) {
  if (!f) return OCTL_E_INVALID;
  QueryTables t;
  OCTL_TRY(query_begin(f, "point_to_plane", &t));
  octl_ctx* ctx = f->ctx;
  PlaneTable pt;
  OCTL_TRY(query_plane_table(f, "point_to_plane", min_points, max_variance, &pt));
  if (query_bad_count(n) || (n > 0 && (!xyz_dev || !node_dev || !row_dev || !distance_dev)))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad point_to_plane arguments");
  if (n == 0) return OCTL_OK;
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return launch_query<true>(ctx, "point_to_plane", xyz_dev, n, t, pt, node_dev, row_dev, distance_dev);
}

}  // extern "C"
