// The lock-free union-find of the plane segments (segments.hip) and of the Euclidean clusters
// (cluster.hip): parent[x] = x for a root, a smaller member of the same tree otherwise, -1 for an entry
// that takes no part.
//
// Why the roots are a function of the input: a union hooks the LARGER of two roots under the smaller with a 32-bit
// compare-and-swap that succeeds only while the larger one still is a root.  parent[x] <= x therefore holds at every
// moment - no cycle can form - every successful hook joins exactly two trees that an edge connects, and a union
// returns only when both ends have one root.  When the kernel ends the trees are the connected components, and the
// root of a tree, having no smaller parent, is its smallest member, whatever the order in which the lanes ran.
//
// Every loop spends from the caller's step budget: an exhausted budget (or an entry that breaks parent[x] <= x - a
// damaged table) returns -1, and the caller sets its error word.  Nothing spins without a bound.  A sound table never
// spends 3 n steps in one union of n entries: a find only moves down (parent[x] < x), a retry follows a hook that took
// the root the union stood on, and both ends go on from where they stand.
//
// __host__ __device__, as nearest_walk.h is: a stand-alone single-threaded host program runs the very linking sink of
// the kernels (tests/host/cluster_host.cpp); the host branch uses plain loads and stores.
#pragma once
#include <cstdint>

#include "common.h"

__host__ __device__ __forceinline__ int32_t uf_load(const int32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// parent[x] = min(parent[x], v)
__host__ __device__ __forceinline__ void uf_lower(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, v);
#else
  if (v < *p) *p = v;
#endif
}

// *p = v when *p == expected; what *p held
__host__ __device__ __forceinline__ int32_t uf_swap(int32_t* p, int32_t expected, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expected, v);
#else
  const int32_t old = *p;
  if (old == expected) *p = v;
  return old;
#endif
}

// root of x, halving the path on the way (a non-root's parent only ever moves to another of its ancestors, so any
// order of these writes keeps parent[x] <= x and the trees); -1 when the table is damaged or the budget is spent
__host__ __device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x, int64_t& budget) {
  for (;;) {
    const int32_t p = uf_load(parent + x);
    if (p == x) return x;
    if (p < 0 || p > x || --budget < 0) return -1;
    const int32_t g = uf_load(parent + p);
    if (g >= 0 && g < p) uf_lower(parent + x, g);
    x = p;
  }
}

// the trees of a and b joined: their common root, or -1 (damaged table, budget spent)
__host__ __device__ __forceinline__ int32_t uf_union(int32_t* parent, int32_t a, int32_t b, int64_t& budget) {
  for (;;) {
    a = uf_find(parent, a, budget);
    b = a < 0 ? -1 : uf_find(parent, b, budget);
    if (a < 0 || b < 0) return -1;
    if (a == b) return a;
    if (a < b) {
      const int32_t s = a;
      a = b;
      b = s;
    }
    if (uf_swap(parent + a, a, b) == a) return b;
    // (someone hooked a first: it is no root any more - find again from where we stand)
    if (--budget < 0) return -1;
  }
}
