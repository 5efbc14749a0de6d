// One query point against the stored points: the walk of octl_forest_nearest (nearest.hip states the definition,
// DESIGN.md 4.11 the argument), shared with the matching kernel of octl_forest_point_registration_system
// (register_points.hip).  The walk visits; what becomes of a candidate is the caller's sink:
//
//   double sink.worst()                          d2 of the last place of the list (+inf while it is free): with r2 the
//                                                bound a cube is skipped by and a candidate is admitted by;
//   void   sink.offer(d2, id, pos)               a stored point with d2 <= min(r2, worst()): id = slot << 32 | index in
//                                                the pose, pos = its row in the ordered arrays (xyz_ord, ord_idx).
//
// One definition, so that both kernels examine the same cubes in the same order and form the same d2 bits.
// __host__ __device__, as cell_walk.h is: a stand-alone host program runs the very walk of the kernels over tables it
// reads from a file (tests/host/moments_host.cpp).
#pragma once
#include "common.h"
#include "forest.h"
#include "query_walk.h"

struct NNTables {
  QueryTables t;
  const int32_t* parent;
  const int32_t* first;    // [n_nodes] first record of the node's run (valid where cnt > 0)
  const int32_t* cnt;      // [n_nodes] selected blocks of the node (0: none, or not a leaf)
  const uint4* rec;        // [selected blocks] in (node, slot) order: {start, size, slot, store offset of the pose}
  const double* xyz_ord;
  const uint32_t* ord_idx;
  int64_t max_steps;       // more cubes than a sound table lets one walk enter and leave: a damaged table ends the walk
};

// nearest.hip.  What a search starts with: the refusals of octl_forest_nearest in its order, under the caller's name
// `what`, then the tables and the block index of the selection - made only when missing or stale
int nearest_begin(octl_forest* f, const char* what, int64_t n, int32_t k, double max_distance, const uint8_t* slot_sel,
                  int32_t n_sel, bool pointers_ok, NNTables* T);
// nearest.hip.  Its tail, for a search with refusals of its own (cell_walk.h: cell_begin): the selection, the refusal of
// displaced rows and, for n > 0, the index and the tables of the walk; T->t is the caller's (query_begin)
int nn_tables(octl_forest* f, const char* what, int64_t n, const uint8_t* slot_sel, int32_t n_sel, NNTables* T);

// A representable lower bound g >= 0 of |fl(q - p)| along one axis for every point p the cube (c, e) can hold.
//
// What placement guarantees (scheme_walk.h, the same comparisons in every build path): for a root and for every split
// node the rounded difference a = fl(p - c) satisfies 0 <= a < e, which is c <= p < c + e in real numbers (fl is
// monotone and 0 and e are representable); a child is chosen by a >= e / 2, and the table holds the child's corner
// as fl(c + e / 2).  So a point of an upper child may lie below that rounded corner, and one of either child above the
// rounded corner + edge, by at most 2^-53 (|c'| + e') of the child (c', e') - half an ulp of each sum.  The same holds
// for fl(c + e) of a non-dyadic single cube.  In real numbers therefore  c - s <= p < c + e + s,  s = 2^-53 (|c| + e).
// The gap is formed with roundings of its own: A = fl(c - q) and U = fl(fl(q - c) - e) differ from the real values by
// at most 2^-53 (|A|) and 2^-53 (|U| + |q - c|), and the subtraction of the slack w rounds once more; all of it is below
// 3 * 2^-53 (|q| + |c| + e), and w = 2^-50 (|q| + |c| + e) is 8 * 2^-53 of that.  g = max(A - w, U - w, 0) is then a
// double that does not exceed |q - p| for any such p, hence (fl monotone, g representable) not |fl(q - p)| either.
__host__ __device__ __forceinline__ double cube_gap(double q, double c, double e) {
  const double w = 0x1p-50 * ((fabs(q) + fabs(c)) + e);
  const double lo = (c - q) - w, hi = ((q - c) - e) - w;
  return fmax(fmax(lo, hi), 0.0);
}

// ... and of d2: squares, and sums of non-negative doubles, are monotone under rounding, so the formula of d2 applied
// to the three gaps in the same order is a lower bound of the d2 the kernel forms for p, rounding included.
__host__ __device__ __forceinline__ double cube_bound(double qx, double qy, double qz, double cx, double cy,
                                                      double cz, double e) {
  const double gx = cube_gap(qx, cx, e), gy = cube_gap(qy, cy, e), gz = cube_gap(qz, cz, e);
  return (gx * gx + gy * gy) + gz * gz;
}

// +inf, for the device and for a host build of the walk (tests/host/moments_host.cpp) alike
__host__ __device__ __forceinline__ double nn_infinity() {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double(0x7ff0000000000000ll);
#else
  return __builtin_inf();
#endif
}

// the child the query would be placed in (any value 0..7 for a query outside the cube: it only orders the visit)
__host__ __device__ __forceinline__ int own_child(double qx, double qy, double qz, double cx, double cy, double cz,
                                                  double e) {
  const double h = e / 2.0;
  return ((qx - cx) >= h ? 4 : 0) | ((qy - cy) >= h ? 2 : 0) | ((qz - cz) >= h ? 1 : 0);
}

__host__ __device__ __forceinline__ bool cand_less(double d, uint64_t id, double bd, uint64_t bid) {
  return d < bd || (d == bd && id < bid);
}

// Every stored point of the index within r of q = (qx, qy, qz), offered to the sink (r2 = fl(r r), formed once on the
// host).  A query that is not finite, and a forest without roots, offer nothing.
template <class Sink>
__host__ __device__ __forceinline__ void nearest_walk(const NNTables& T, double qx, double qy, double qz, double r,
                                                      double r2, Sink& sink) {
  const double INF = nn_infinity();
  const QueryTables& t = T.t;
  const bool finite = fabs(qx) < INF && fabs(qy) < INF && fabs(qz) < INF;  // (false for NaN)
  if (!(finite && t.V > 0)) return;
  // voxels the ball can reach, own voxel first.  The range is taken from q -+ (r + slack): fl(dx dx) <= fl(r r)
  // does not exclude |dx| one ulp above r.  A single cube is the one "voxel" (0, 0, 0) of its key.
  int64_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, own[3] = {0, 0, 0};
  bool any = true, own_ok = true;
  if (t.mode == 0) {
    const double q[3] = {qx, qy, qz};
    const int32_t org[3] = {t.org.x, t.org.y, t.org.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double w = r + 0x1p-50 * (fabs(q[a]) + r);
      // (indices outside the key window or beyond the absolute limit have no root: clamped away)
      const double wmin = fmax(-(double)OCTL_VOX_ABS_LIMIT + 1.0, (double)org[a] - (double)OCTL_VOX_BIAS + 1.0);
      const double wmax = fmin((double)OCTL_VOX_ABS_LIMIT - 1.0, (double)org[a] + (double)OCTL_VOX_BIAS - 1.0);
      const double fl = fmax(floor_div_exact(q[a] - w, t.L), wmin);
      const double fh = fmin(floor_div_exact(q[a] + w, t.L), wmax);
      const double fo = floor_div_exact(q[a], t.L);
      if (!(fl <= fh)) any = false;
      own_ok = own_ok && fo >= fl && fo <= fh;
      lo[a] = (int64_t)fl;
      hi[a] = (int64_t)fh;
      own[a] = (int64_t)fo;
    }
  }
  const uint64_t own_code = own_ok ? vkey_pack(own[0], own[1], own[2], t.org) : ~0ull;
  int64_t steps = 0;
  for (int pass = own_ok ? 0 : 1; any && pass < 2; ++pass) {
    const int64_t x0 = pass ? lo[0] : own[0], x1 = pass ? hi[0] : own[0];
    const int64_t y0 = pass ? lo[1] : own[1], y1 = pass ? hi[1] : own[1];
    const int64_t z0 = pass ? lo[2] : own[2], z1 = pass ? hi[2] : own[2];
    for (int64_t vx = x0; vx <= x1; ++vx) {
      for (int64_t vy = y0; vy <= y1; ++vy) {
        // (z is the lowest field of the key: the voxels of one column are consecutive codes)
        const uint64_t code0 = vkey_pack(vx, vy, z0, t.org), code1 = vkey_pack(vx, vy, z1, t.org);
        for (int64_t rr = lower_bound_u64(t.vcode, t.V, code0); rr < t.V; ++rr) {
          const uint64_t code = t.vcode[rr];
          if (code > code1) break;
          if (pass && code == own_code) continue;
          // ---- the tree under root rr, depth first without a stack ----
          const int32_t root = (int32_t)rr;
          int32_t node = root;
          for (;;) {
            if (++steps > T.max_steps) break;
            const double cx = t.corner[3 * (int64_t)node + 0], cy = t.corner[3 * (int64_t)node + 1],
                         cz = t.corner[3 * (int64_t)node + 2], e = t.edge[node];
            const double cur = fmin(r2, sink.worst());
            // (skipped only when the bound is ABOVE the k-th best: a cube that can hold a tie is examined)
            if (!(cur < cube_bound(qx, qy, qz, cx, cy, cz, e))) {
              const int32_t fc = t.first_child[node];
              if (fc >= 0) {
                node = fc + own_child(qx, qy, qz, cx, cy, cz, e);  // (rank 0 of the visiting order below)
                continue;
              }
              const int32_t nrun = T.cnt[node];
              const int32_t run0 = nrun > 0 ? T.first[node] : 0;
              for (int32_t b = 0; b < nrun; ++b) {
                const uint4 rec = T.rec[run0 + b];
                const double* __restrict__ p = T.xyz_ord + 3 * (int64_t)rec.x;
                for (uint32_t j = 0; j < rec.y; ++j, p += 3) {
                  const double dx = qx - p[0], dy = qy - p[1], dz = qz - p[2];
                  const double d2 = (dx * dx + dy * dy) + dz * dz;
                  if (d2 <= fmin(r2, sink.worst())) {
                    const uint64_t id = ((uint64_t)rec.z << 32) | (uint64_t)(T.ord_idx[(int64_t)rec.x + j] - rec.w);
                    sink.offer(d2, id, rec.x + j);
                  }
                }
              }
            }
            // next cube: the siblings in the order (child number XOR own child of the parent), then up
            bool done = false;
            for (;;) {
              if (node == root) {
                done = true;
                break;
              }
              const int32_t par = T.parent[node];
              if (par < 0 || ++steps > T.max_steps) {
                done = true;
                break;
              }
              const int32_t fcp = t.first_child[par];
              const int oc = own_child(qx, qy, qz, t.corner[3 * (int64_t)par + 0], t.corner[3 * (int64_t)par + 1],
                                       t.corner[3 * (int64_t)par + 2], t.edge[par]);
              const int rank = (node - fcp) ^ oc;
              if (rank >= 0 && rank < 7) {
                node = fcp + ((rank + 1) ^ oc);
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
}

// the K best so far, ascending (d2, id); free places hold (inf, all ones).  The two arrays are the
// caller's own locals: the sink only refers to them (nearest.hip says what the compiler makes of the alternative)
template <int KT>
struct NNBest {
  double (&bd)[KT];
  uint64_t (&bid)[KT];
  __device__ __forceinline__ void clear() {
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      bd[j] = INF;
      bid[j] = ~0ull;
    }
  }
  __device__ __forceinline__ double worst() const { return bd[KT - 1]; }
  __device__ __forceinline__ void offer(double d2, uint64_t id, uint32_t) {
    if (cand_less(d2, id, bd[KT - 1], bid[KT - 1])) {
#pragma unroll
      for (int m = KT - 1; m >= 1; --m) {
        const bool up = cand_less(d2, id, bd[m - 1], bid[m - 1]);
        const bool here = cand_less(d2, id, bd[m], bid[m]);
        bd[m] = up ? bd[m - 1] : (here ? d2 : bd[m]);
        bid[m] = up ? bid[m - 1] : (here ? id : bid[m]);
      }
      if (cand_less(d2, id, bd[0], bid[0])) {
        bd[0] = d2;
        bid[0] = id;
      }
    }
  }
};
