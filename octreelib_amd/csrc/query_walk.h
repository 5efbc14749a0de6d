// What the read-only queries share (query.hip: k_query; register.hip: k_reg_partial): the tables a query reads, the
// leaf of one point (locate_one) and the point's residual against the pooled plane of that leaf (plane_residual).
// One definition, so that the registration kernel's node / row / residual are the bits octl_forest_point_to_plane
// answers - by construction, not by a copy that has to be kept in step.
#pragma once
#include <algorithm>

#include "common.h"
#include "forest.h"
#include "scheme_walk.h"

struct QueryTables {
  int mode;
  double L;
  VoxOrg org;
  const uint64_t* vcode;
  int64_t V;
  const int32_t* first_child;
  const double* corner;
  const double* edge;
};

struct PlaneTable {
  const int32_t* node_row;  // [n_nodes] row of the pooled table, -1: the leaf holds no pooled point
  const double2* rows;      // [n_rows][4]: {nx, ny}, {nz, mx}, {my, mz}, {lambda0, count}
  int32_t min_points;
  double max_variance;      // < 0: no variance test
};

__device__ __forceinline__ int32_t locate_one(const QueryTables& t, double px, double py, double pz) {
  if (t.V <= 0) return -1;  // (a forest without points has no root)
  if (t.mode == 1) {
    // a single cube has no voxel to miss: a point outside it (or not finite) has no leaf, whether or not the root
    // is split (the walk itself only looks at the cubes of split nodes, as the insertion does)
    const double e = t.edge[0];
    const double ax = px - t.corner[0], ay = py - t.corner[1], az = pz - t.corner[2];
    if (!((ax >= 0.0) && (ax < e) && (ay >= 0.0) && (ay < e) && (az >= 0.0) && (az < e))) return -1;
  }
  int32_t node = -1;
  uint64_t code = 0;
  const int status = scheme_walk(px, py, pz, t.mode, t.L, t.org, t.vcode, t.V, t.first_child, t.corner, t.edge, &node,
                                 &code);
  return status == WALK_LEAF ? node : -1;
}

// row of the pooled table that answers for `node` (-1: no leaf, no pooled point, too few of them, too thick) and the
// signed distance of p to its plane (NaN where the row is -1); nrm[3] = the plane's normal where the row is >= 0
__device__ __forceinline__ double plane_residual(const PlaneTable& pt, int32_t node, double px, double py, double pz,
                                                 int32_t* row_out, double nrm[3]) {
  int32_t row = node >= 0 ? pt.node_row[node] : -1;
  double d = __longlong_as_double(0x7ff8000000000000ll);
  if (row >= 0) {
    const double2* r = pt.rows + 4 * (int64_t)row;
    const double2 a = r[0], b = r[1], c = r[2], w = r[3];
    const bool keep = w.y >= (double)pt.min_points && !(pt.max_variance >= 0.0 && w.x > pt.max_variance);
    if (keep) {
      const double dx = px - b.y, dy = py - c.x, dz = pz - c.y;
      d = fma(a.x, dx, fma(a.y, dy, b.x * dz));
      nrm[0] = a.x;
      nrm[1] = a.y;
      nrm[2] = b.x;
    } else {
      row = -1;
    }
  }
  *row_out = row;
  return d;
}

// query.hip.  What every query starts with: the forest is settled, built, and its voxel codes are on the device ...
int query_begin(octl_forest* f, const char* what, QueryTables* t);
// ... and the pooled plane table is the one of the forest as it stands (OCTL_E_STATE with the cause otherwise)
int query_plane_table(octl_forest* f, const char* what, int32_t min_points, double max_variance, PlaneTable* pt);
static inline bool query_bad_count(int64_t n) { return n < 0 || n >= ((int64_t)1 << 31); }

// nearest.hip.  f->nn_tab, the index node -> run of selected (leaf, pose) blocks that octl_forest_nearest searches and
// octl_forest_raycast takes a leaf's occupancy from: [record uint4 per block | first i32 per node | count i32 per node]
struct NNTab {
  size_t nb, n_nodes;  // (at least one of each)
  Carve plan;
  Carve::Part<uint4> rec = plan.add<uint4>(nb);
  Carve::Part<int32_t> first = plan.add<int32_t>(n_nodes), cnt = plan.add<int32_t>(n_nodes);
  constexpr NNTab(int64_t blocks, int64_t nodes)
      : nb((size_t)std::max<int64_t>(blocks, 1)), n_nodes((size_t)std::max<int64_t>(nodes, 1)) {}
};
static_assert(NNTab(100, 10).cnt.off == 2048 && NNTab(100, 10).plan.total == 2304, "NNTab offsets");
// ... made for the selection `sel` (empty: every pose) of the forest as it stands; stamps f->nn_stamp, keeps f->nn_sel
int nn_prepare(octl_forest* f, const std::vector<uint8_t>& sel);
