// One query against the stored points of one cell of a regular lattice: the walk of octl_forest_cell_count and of
// octl_forest_thin (cell.hip states the definition, DESIGN.md 4.22 the argument).  A sibling of nearest_walk: the same
// NNTables, the same stackless traversal under every root, a box prune in the place of the ball prune.  __host__
// __device__, so that a stand-alone host program can run the very code of the kernels over tables it reads from a file
// (tests/host/cell_host.cpp: a CPU build under the sanitizers, compared with cell_count_np).  What becomes of a
// candidate is the caller's sink:
//
//   void sink.offer(idx, pos)   a stored point of the query's cell: idx = its index in the point store - poses in slot
//                               order, rows in insertion order, so idx orders the stored points as (slot, index in the
//                               pose) does - pos = its row in the ordered arrays (xyz_ord, ord_idx);
//   bool sink.full()            the count is saturated: the walk ends.
#pragma once
#include <cmath>

#include "nearest_walk.h"

// the lattice is absolute: cell index k = floor(p / cell) per axis, the floor of the TRUE quotient (ref_arith.h:
// floor_div_exact, np.floor_divide).  Every stored point has |k| < 2^50 (cell_begin refuses a cell that is too small for
// the map's domain), so k and k + 1 are exact doubles and a query beyond that shares its cell with no stored point.
#define CELL_INDEX_LIMIT 0x1p50

struct CellBox {
  double k[3], k1[3];   // the cell's index and index + 1, exact
  double lo[3], hi[3];  // fl(k cell), fl((k + 1) cell): the cell's faces, each within half an ulp of its place
};

// q lies in [k cell, (k + 1) cell) in real numbers.  fma rounds the exact q - k cell once; that difference is a
// multiple of 2^-1074 (k is an integer, cell and q are doubles), so it is zero or at least the smallest denormal in
// magnitude and its sign survives the rounding - provided f64 denormals are not flushed, and they are not.  The same
// test as floor_div_exact(q, cell) == k, without the division.
__host__ __device__ __forceinline__ bool cell_holds(double q, double k, double k1, double cell) {
  return fma(-k, cell, q) >= 0.0 && fma(-k1, cell, q) < 0.0;
}

// May the cube (c, e) hold a point of [K_lo, K_hi) = [k cell, (k + 1) cell) along one axis?  false ONLY when it cannot.
//
// What a cube can hold (nearest_walk.h: cube_gap has the argument): c - s <= p < c + e + s, s = 2^-53 (|c| + e), in real
// numbers.  So nothing of the cube lies in the cell when c + e + s <= K_lo (all of it below) or c - s >= K_hi (all of it
// at or above the upper face, which is not part of the cell).  The code forms
//   U = fl(lo - fl(c + e))   against K_lo - (c + e):  fl(c + e) is off by at most 2^-53 (|c| + e), lo = fl(k cell) by
//                            2^-53 |lo|, the difference rounds once more, by 2^-53 |U| <= 2^-53 (|lo| + |c| + e)(1 + 2^-52):
//                            together below 2^-51 (|lo| + |c| + e);
//   A = fl(c - hi)           against c - K_hi:  hi is off by 2^-53 |hi|, the difference by 2^-53 (|c| + |hi|):
//                            together below 2^-52 (|hi| + |c|).
// With s on top either error stays below 0.7 w for w = 2^-50 (max(|lo|, |hi|) + |c| + e) (formed with three roundings
// of its own, 2^-51 w at most).  U > w therefore means K_lo - (c + e) > s and A > w means c - K_hi > s: the cube is
// skipped only when it holds nothing of the cell.  Anything closer is examined, which only costs time.
__host__ __device__ __forceinline__ bool cube_meets_axis(double lo, double hi, double c, double e) {
  const double w = 0x1p-50 * ((fmax(fabs(lo), fabs(hi)) + fabs(c)) + e);
  return !((lo - (c + e)) > w || (c - hi) > w);
}

__host__ __device__ __forceinline__ bool cube_meets_cell(const CellBox& b, double cx, double cy, double cz, double e) {
  return cube_meets_axis(b.lo[0], b.hi[0], cx, e) && cube_meets_axis(b.lo[1], b.hi[1], cy, e) &&
         cube_meets_axis(b.lo[2], b.hi[2], cz, e);
}

// Every stored point of the index that lies in the lattice cell of q = (qx, qy, qz), offered to the sink until it is
// full.  A query that is not finite, one whose cell index is not below 2^50 in magnitude and a forest without roots
// offer nothing.  The order of the visit is the order of the table (children 0 .. 7): a count does not depend on it.
template <class Sink>
__host__ __device__ __forceinline__ void cell_walk(const NNTables& T, double qx, double qy, double qz, double cell,
                                                   Sink& sink) {
  const QueryTables& t = T.t;
  const double q[3] = {qx, qy, qz};
  CellBox box;
  bool ok = t.V > 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // (NaN and +-inf give an index that is not below the limit: every comparison with NaN is false)
    const double k = floor_div_exact(q[a], cell);
    ok = ok && fabs(k) < CELL_INDEX_LIMIT;
    box.k[a] = k;
    box.k1[a] = k + 1.0;
    box.lo[a] = k * cell;
    box.hi[a] = (k + 1.0) * cell;
  }
  if (!ok || sink.full()) return;
  // The top-level voxels the cell can touch.  A stored point of voxel v has v L <= p < (v + 1) L exactly (its voxel is
  // floor_div_exact(p, L)), and one of the cell K_lo <= p < K_hi: v lies between floor(K_lo / L) and floor(K_hi / L).
  // The range is taken from the rounded faces -+ 2^-50 of their size, which is more than their half ulp.  With
  // cell <= L that is two voxels per axis, three where both faces lie on walls; the loops are bounded whatever the
  // arithmetic did.  A single cube is the one "voxel" (0, 0, 0) of its key.
  int64_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (t.mode == 0) {
    const int32_t org[3] = {t.org.x, t.org.y, t.org.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double w = 0x1p-50 * (fmax(fabs(box.lo[a]), fabs(box.hi[a])) + cell);
      // (indices outside the key window or beyond the absolute limit have no root: clamped away)
      const double wmin = fmax(-(double)OCTL_VOX_ABS_LIMIT + 1.0, (double)org[a] - (double)OCTL_VOX_BIAS + 1.0);
      const double wmax = fmin((double)OCTL_VOX_ABS_LIMIT - 1.0, (double)org[a] + (double)OCTL_VOX_BIAS - 1.0);
      const double fl = fmax(floor_div_exact(box.lo[a] - w, t.L), wmin);
      const double fh = fmin(fmin(floor_div_exact(box.hi[a] + w, t.L), wmax), fl + 3.0);
      if (!(fl <= fh)) return;
      lo[a] = (int64_t)fl;
      hi[a] = (int64_t)fh;
    }
  }
  int64_t steps = 0;
  for (int64_t vx = lo[0]; vx <= hi[0]; ++vx) {
    for (int64_t vy = lo[1]; vy <= hi[1]; ++vy) {
      // (z is the lowest field of the key: the voxels of one column are consecutive codes)
      const uint64_t code0 = vkey_pack(vx, vy, lo[2], t.org), code1 = vkey_pack(vx, vy, hi[2], t.org);
      for (int64_t rr = lower_bound_u64(t.vcode, t.V, code0); rr < t.V; ++rr) {
        if (t.vcode[rr] > code1) break;
        // ---- the tree under root rr, depth first without a stack (nearest_walk.h) ----
        const int32_t root = (int32_t)rr;
        int32_t node = root;
        for (;;) {
          if (++steps > T.max_steps) return;
          const double cx = t.corner[3 * (int64_t)node + 0], cy = t.corner[3 * (int64_t)node + 1],
                       cz = t.corner[3 * (int64_t)node + 2], e = t.edge[node];
          if (cube_meets_cell(box, cx, cy, cz, e)) {
            const int32_t fc = t.first_child[node];
            if (fc >= 0) {
              node = fc;
              continue;
            }
            const int32_t nrun = T.cnt[node];
            const int32_t run0 = nrun > 0 ? T.first[node] : 0;
            for (int32_t b = 0; b < nrun; ++b) {
              const uint4 rec = T.rec[run0 + b];
              const double* __restrict__ p = T.xyz_ord + 3 * (int64_t)rec.x;
              for (uint32_t j = 0; j < rec.y; ++j, p += 3) {
                if (cell_holds(p[0], box.k[0], box.k1[0], cell) && cell_holds(p[1], box.k[1], box.k1[1], cell) &&
                    cell_holds(p[2], box.k[2], box.k1[2], cell)) {
                  sink.offer(T.ord_idx[(int64_t)rec.x + j], rec.x + j);
                  if (sink.full()) return;
                }
              }
            }
          }
          // next cube: the next sibling, then up
          bool done = false;
          for (;;) {
            if (node == root) {
              done = true;
              break;
            }
            const int32_t par = T.parent[node];
            if (par < 0 || ++steps > T.max_steps) return;
            const int rank = node - t.first_child[par];
            if (rank >= 0 && rank < 7) {
              ++node;
              break;
            }
            node = par;
          }
          if (done) break;
        }
      }
    }
  }
}

// cell.hip.  What a cell query starts with: the refusals of octl_forest_cell_count in its order, under the
// caller's name `what`, then the tables and the block index of the selection - made only when missing or stale
int cell_begin(octl_forest* f, const char* what, int64_t n, double cell, const uint8_t* slot_sel, int32_t n_sel,
               bool pointers_ok, NNTables* T);
