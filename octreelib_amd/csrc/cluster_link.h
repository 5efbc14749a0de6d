// The linking sink of the Euclidean clusters (cluster.hip): the walk of octl_forest_radius_count
// (nearest_walk.h: the same cubes in the same order, the same d2 bits) with a sink that JOINS instead of counting.  The
// vertices are positions of the ordered arrays; an edge is d2 <= r2, inclusive, and d2 is symmetric bit for bit
// (dx = q_x - p_x is negated exactly, the squares are equal), so every edge is seen from both ends and is taken from
// the larger one only.
//
// __host__ __device__, as the walk is: tests/host/cluster_host.cpp runs this very sink on the CPU.
#pragma once
#include "nearest_walk.h"
#include "union_find.h"

// worst() is always +inf: nothing prunes below r2 and every stored point within the radius is offered.  self: the
// position the walk runs for; root: a root `self` has been seen under - a member of self's tree for ever, trees only
// merge - kept in a register: a candidate whose parent IS that entry shares the tree already and costs one load, which
// is what most of a dense neighbourhood does once the first few unions have run.  failed: a union ran out of its
// budget (the caller sets the error word).
struct ClusterLink {
  int32_t* parent;
  int32_t self, root;
  int64_t max_steps;
  bool failed;
  __host__ __device__ __forceinline__ double worst() const { return nn_infinity(); }
  __host__ __device__ __forceinline__ void offer(double, uint64_t, uint32_t pos) {
    if ((int32_t)pos >= self || failed) return;
    if (uf_load(parent + pos) == root) return;
    int64_t budget = max_steps;
    const int32_t joined = uf_union(parent, root, (int32_t)pos, budget);
    if (joined < 0) failed = true;
    else root = joined;
  }
};

// every edge of position `self` to a smaller position, joined; false: a union ran out of its budget
__host__ __device__ __forceinline__ bool cluster_link_one(const NNTables& T, int32_t* parent, int32_t self, double r,
                                                          double r2, int64_t max_steps) {
  const double* q = T.xyz_ord + 3 * (int64_t)self;
  ClusterLink sink = {parent, self, self, max_steps, false};
  nearest_walk(T, q[0], q[1], q[2], r, r2, sink);
  return !sink.failed;
}
