// One point -> its leaf of the scheme: the walk shared by the incremental insertion (incremental.hip: k_inc_place,
// which places the points of a late pose) and the read-only queries (query.hip), so that a query answers with
// exactly the leaf an inserted point would land in - boundary points included - by construction.
//
// voxel (grid/grid.py:72-76) by floor_div_exact, root by binary search over the sorted packed voxel codes, then down
// the node table (octree/octree.py:67-100: idx = floor((p - corner) / (edge / 2)) per axis, child 4 ix + 2 iy + iz,
// restated as exact comparisons on the same rounded differences, see compute_path in build.hip).
#pragma once
#include "forest.h"
#include "ref_arith.h"

__host__ __device__ __forceinline__ int64_t lower_bound_u64(const uint64_t* __restrict__ a, int64_t n, uint64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

enum {
  WALK_LEAF = 0,     // *node is the leaf that holds the point
  WALK_DOMAIN = 1,   // not finite, or a voxel outside the domain of the packed keys (grid mode only)
  WALK_MISS = 2,     // the scheme has no root for the point's voxel; *code is that voxel's packed key
  WALK_OUTSIDE = 3,  // outside the cube of a node that is split (*node); the reference raises IndexError or picks a
                     // wrong child there
  WALK_DEEP = 4      // more than 64 levels: a damaged table (children are numbered behind their parents, so a sound
                     // one ends the walk)
};

__device__ __forceinline__ int scheme_walk(double px, double py, double pz, int mode, double L, const VoxOrg& org,
                                           const uint64_t* __restrict__ vcode, int64_t V,
                                           const int32_t* __restrict__ first_child,
                                           const double* __restrict__ corner, const double* __restrict__ edge,
                                           int32_t* node_out, uint64_t* code_out) {
  int qx = 0, qy = 0, qz = 0;
  if (mode == 0) {
    const double fx = floor_div_exact(px, L), fy = floor_div_exact(py, L), fz = floor_div_exact(pz, L);
    const double lim = (double)OCTL_VOX_ABS_LIMIT;
    if (!((fabs(fx) < lim) && (fabs(fy) < lim) && (fabs(fz) < lim) &&
          vkey_in_window((int64_t)fx, (int64_t)fy, (int64_t)fz, org)))  // also NaN
      return WALK_DOMAIN;
    qx = (int)fx;
    qy = (int)fy;
    qz = (int)fz;
  }
  const uint64_t code = vkey_pack(qx, qy, qz, org);
  *code_out = code;
  const int64_t r = lower_bound_u64(vcode, V, code);
  if (r >= V || vcode[r] != code) return WALK_MISS;
  int32_t node = (int32_t)r;
  int32_t fc = first_child[node];
  int status = WALK_LEAF;
  for (int depth = 0; fc >= 0; ++depth) {
    if (depth >= 64) {
      status = WALK_DEEP;
      break;
    }
    const double cx = corner[3 * (int64_t)node + 0], cy = corner[3 * (int64_t)node + 1],
                 cz = corner[3 * (int64_t)node + 2], e = edge[node];
    const double h = e / 2.0;
    const double ax = px - cx, ay = py - cy, az = pz - cz;
    const bool ok = (ax >= 0.0) && (ax < e) && (ay >= 0.0) && (ay < e) && (az >= 0.0) && (az < e);
    if (!ok) {
      status = WALK_OUTSIDE;
      break;
    }
    node = fc + ((ax >= h ? 4 : 0) | (ay >= h ? 2 : 0) | (az >= h ? 1 : 0));
    fc = first_child[node];
  }
  *node_out = node;
  return status;
}
