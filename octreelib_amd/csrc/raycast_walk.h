// One ray against the scheme: the traversal of octl_forest_raycast (raycast.hip states the definition, DESIGN.md 4.14
// the argument) and, further down, that of octl_forest_ray_evidence (evidence.hip).  __host__
// __device__, so that a stand-alone host program can run the very code of the kernel over tables it reads from a file
// (tests/host/raycast_host.cpp, tests/host/evidence_host.cpp: CPU builds under the sanitizers, compared with raycast_np
// and ray_evidence_np).
#pragma once
#include <cmath>

#include "query_walk.h"

// a grid-mode ray spans at most this many voxel edges, and lies within 2^40 of them of the origin of t
#define RAY_CAP_EDGES 256.0
#define RAY_T_LIMIT 0x1p40

struct RayTables {
  QueryTables t;
  const int32_t* parent;
  const int32_t* first;  // the index of nearest.hip (cube form): run of selected blocks of a node ...
  const int32_t* cnt;
  const uint4* rec;      // ... {start, size, slot, store offset of the pose}
  PlaneTable pt;         // (plane form)
  int32_t min_points;
  int64_t max_steps;     // more cubes than a sound table lets one ray enter and leave: a damaged table ends the walk
};

struct Ray {
  double ox, oy, oz, dx, dy, dz, ix, iy, iz, t_min, t_max;
  bool zx, zy, zz;  // the axis bounds nothing: d == 0 or 1 / d not finite
};

// One axis of the interval of the box [lo, hi]: false when the axis bounds nothing and o is outside [lo, hi].
// x -> fl(fl(x - o) inv) is monotone (a rounded difference and a rounded product with a fixed factor are), rising for
// inv > 0 and falling for inv < 0.  So for lo' <= lo and hi <= hi' the near value of [lo', hi'] is <= that of [lo, hi]
// and its far value >=, whatever the sign of inv - and lo' <= lo <= o <= hi <= hi' on an axis that bounds nothing.
__host__ __device__ __forceinline__ bool ray_axis(double lo, double hi, double o, double inv, bool zero, double& t_in,
                                         double& t_out) {
  if (zero) return lo <= o && o <= hi;
  const double a = (lo - o) * inv, b = (hi - o) * inv;
  t_in = fmax(t_in, fmin(a, b));
  t_out = fmin(t_out, fmax(a, b));
  return true;
}

// The slack that makes the box of an inner node (c, e) contain the box [c', fl(c' + e')] of every leaf below it, per
// face: w = 2^-45 (|c| + e).
//   below: a child's corner is c or fl(c + e / 2) >= c (fl monotone), so by induction c' >= c >= fl(c - w);
//   above: each level rounds one sum, off by at most h = 2^-53 (|c| + e) (1 + 2^-52) - half an ulp of a value inside
//          the node - so after j <= 64 levels (a deeper table is a damaged one: scheme_walk.h) c' is within j h of
//          its exact place, fl(c' + e') within (j + 1) h of a value <= c + e, and fl(c + e) within h of that:
//          fl(c' + e') <= fl(c + e) + 66 h < fl(fl(c + e) + w), as w = 256 * 2^-53 (|c| + e).
// A leaf is its own box: w = 0 gives lo = c and hi = fl(c + e), the definition's bits.
__host__ __device__ __forceinline__ bool ray_box(const Ray& r, double cx, double cy, double cz, double e, bool leaf,
                                        double& t_in, double& t_out) {
  const double s = leaf ? 0.0 : 0x1p-45;
  const double wx = s * (fabs(cx) + e), wy = s * (fabs(cy) + e), wz = s * (fabs(cz) + e);
  t_in = r.t_min;
  t_out = r.t_max;
  bool ok = ray_axis(cx - wx, (cx + e) + wx, r.ox, r.ix, r.zx, t_in, t_out);
  ok = ray_axis(cy - wy, (cy + e) + wy, r.oy, r.iy, r.zy, t_in, t_out) && ok;
  ok = ray_axis(cz - wz, (cz + e) + wz, r.oz, r.iz, r.zz, t_in, t_out) && ok;
  return ok && t_in <= t_out;
}

struct RayBest {
  double t;
  int32_t node, row;
};

__host__ __device__ __forceinline__ bool ray_less(double t, int32_t node, const RayBest& b) {
  return t < b.t || (t == b.t && node < b.node);
}

// the tree under `root`, depth first without a stack (nearest.hip: k_nearest), children in the order child number XOR
// mask, mask = the axes along which the ray travels down: front to back for every ray of these signs
template <bool PLANE>
__host__ __device__ __forceinline__ void ray_walk(const RayTables& T, const Ray& r, int mask, int32_t root, int64_t& steps,
                                         RayBest& best) {
  const QueryTables& t = T.t;
  int32_t node = root;
  for (;;) {
    if (++steps > T.max_steps) return;
    const double cx = t.corner[3 * (int64_t)node + 0], cy = t.corner[3 * (int64_t)node + 1],
                 cz = t.corner[3 * (int64_t)node + 2], e = t.edge[node];
    const int32_t fc = t.first_child[node];
    double t_in, t_out;
    // (skipped only when the box is not crossed or is entered ABOVE the best hit: a cube that can hold a tie is examined)
    if (ray_box(r, cx, cy, cz, e, fc < 0, t_in, t_out) && !(t_in > best.t)) {
      if (fc >= 0) {
        node = fc + mask;  // (rank 0 of the visiting order below)
        continue;
      }
      if (PLANE) {
        const int32_t row = T.pt.node_row[node];
        if (row >= 0) {
          const double2* p = T.pt.rows + 4 * (int64_t)row;
          const double2 a = p[0], b = p[1], c = p[2], w = p[3];
          if (w.y >= (double)T.pt.min_points && !(T.pt.max_variance >= 0.0 && w.x > T.pt.max_variance)) {
            const double num = (a.x * (b.y - r.ox) + a.y * (c.x - r.oy)) + b.x * (c.y - r.oz);
            const double den = (a.x * r.dx + a.y * r.dy) + b.x * r.dz;
            const double th = num / den;
            if (den != 0.0 && t_in <= th && th <= t_out && ray_less(th, node, best)) {
              best.t = th;
              best.node = node;
              best.row = row;
            }
          }
        }
      } else if (ray_less(t_in, node, best)) {
        const int32_t nrun = T.cnt[node];
        const int32_t run0 = nrun > 0 ? T.first[node] : 0;
        int64_t held = 0;
        for (int32_t b = 0; b < nrun; ++b) held += (int64_t)T.rec[run0 + b].y;
        if (held >= (int64_t)T.min_points) {
          best.t = t_in;
          best.node = node;
        }
      }
    }
    // next cube: the siblings in the order (child number XOR mask), then up
    for (;;) {
      if (node == root) return;
      const int32_t par = T.parent[node];
      if (par < 0 || ++steps > T.max_steps) return;
      const int32_t fcp = t.first_child[par];
      const int rank = (node - fcp) ^ mask;
      if (rank >= 0 && rank < 7) {
        node = fcp + ((rank + 1) ^ mask);
        break;
      }
      node = par;
    }
  }
}

// The voxels along an axis that can hold a crossed leaf while t runs over [ta, tb]: a crossed leaf has
// near <= t_out <= tb and far >= t_in >= ta, which bounds its faces by the ray's positions at ta and tb up to a
// few roundings of (|o| + |t d| + L) 2^-53 each - of the interval arithmetic, of the positions formed here, and
// of the leaf's faces against its voxel's (ray_box); the range is taken 2^-45 of that wide, and the slack being
// strictly larger than the error keeps the voxel below a face the ray only touches.  (Shared by the two marches below;
// in scope where it is used: o3, d3 = the ray's origin and direction, L, wmin, wmax = the window of voxel indices.)
#define RAY_RANGE(a, ta, tb, first, last)                                                 \
  do {                                                                                    \
    const double pa = o3[a] + (ta) * d3[a], pb = o3[a] + (tb) * d3[a];                    \
    const double sg = 0x1p-45 * (((fabs(o3[a]) + fabs((ta) * d3[a])) + fabs((tb) * d3[a])) + L); \
    first = fmax(floor_div_exact(fmin(pa, pb) - sg, L), wmin[a]);                         \
    last = fmin(floor_div_exact(fmax(pa, pb) + sg, L), wmax[a]);                          \
  } while (0)

// what the ray o + t d, t_min <= t <= t_max hits first (node -1, t +inf, row -1: nothing, or a dead ray)
template <bool PLANE>
__host__ __device__ __forceinline__ RayBest ray_cast(const RayTables& T, const double* __restrict__ o,
                                                     const double* __restrict__ d, double t_min, double t_max) {
  const double INF = HUGE_VAL;
  const QueryTables& t = T.t;
  Ray r;
  r.ox = o[0], r.oy = o[1], r.oz = o[2];
  r.dx = d[0], r.dy = d[1], r.dz = d[2];
  r.t_min = t_min, r.t_max = t_max;
  r.ix = 1.0 / r.dx, r.iy = 1.0 / r.dy, r.iz = 1.0 / r.dz;
  r.zx = r.dx == 0.0 || !(fabs(r.ix) < INF);
  r.zy = r.dy == 0.0 || !(fabs(r.iy) < INF);
  r.zz = r.dz == 0.0 || !(fabs(r.iz) < INF);
  RayBest best = {INF, -1, -1};
  // (every comparison is false for NaN)
  bool live = fabs(r.ox) < INF && fabs(r.oy) < INF && fabs(r.oz) < INF && fabs(r.dx) <= 1.0 && fabs(r.dy) <= 1.0 &&
              fabs(r.dz) <= 1.0 && fabs(r.t_min) < INF && fabs(r.t_max) < INF && r.t_min <= r.t_max &&
              !(r.zx && r.zy && r.zz) && t.V > 0;
  const int mask = (r.dx < 0.0 ? 4 : 0) | (r.dy < 0.0 ? 2 : 0) | (r.dz < 0.0 ? 1 : 0);
  int64_t steps = 0;
  if (live && t.mode != 0) {
    ray_walk<PLANE>(T, r, mask, 0, steps, best);  // a single cube is the one root
  } else if (live && r.t_max - r.t_min <= RAY_CAP_EDGES * t.L && fabs(r.t_min) <= RAY_T_LIMIT * t.L &&
             fabs(r.t_max) <= RAY_T_LIMIT * t.L) {
    // (a ray above the cap is refused by the host form; here it finds nothing)
    const double L = t.L;
    const double adx = fabs(r.dx), ady = fabs(r.dy), adz = fabs(r.dz);
    const int m = (adx >= ady && adx >= adz) ? 0 : (ady >= adz ? 1 : 2);  // the major axis: at most 256 + 3 slabs
    const double om = m == 0 ? r.ox : m == 1 ? r.oy : r.oz, dm = m == 0 ? r.dx : m == 1 ? r.dy : r.dz;
    const double im = m == 0 ? r.ix : m == 1 ? r.iy : r.iz;
    const double o3[3] = {r.ox, r.oy, r.oz}, d3[3] = {r.dx, r.dy, r.dz};
    const int32_t g3[3] = {t.org.x, t.org.y, t.org.z};
    // voxel indices outside the key window or beyond the absolute limit have no root: clamped away
    double wmin[3], wmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      wmin[a] = fmax(-(double)OCTL_VOX_ABS_LIMIT + 1.0, (double)g3[a] - (double)OCTL_VOX_BIAS + 1.0);
      wmax[a] = fmin((double)OCTL_VOX_ABS_LIMIT - 1.0, (double)g3[a] + (double)OCTL_VOX_BIAS - 1.0);
    }
    double s_lo, s_hi;
    {
      double f0[3], f1[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) RAY_RANGE(a, r.t_min, r.t_max, f0[a], f1[a]);
      s_lo = m == 0 ? f0[0] : m == 1 ? f0[1] : f0[2];
      s_hi = m == 0 ? f1[0] : m == 1 ? f1[1] : f1[2];
    }
    // (|d| <= 1 and the cap: at most 256 + 3 slabs; the bound guards the loop whatever the arithmetic did)
    const int64_t n_slabs = s_lo <= s_hi ? (int64_t)fmin(s_hi - s_lo + 1.0, RAY_CAP_EDGES + 8.0) : 0;
    for (int64_t k = 0; k < n_slabs; ++k) {
      const double sv = dm > 0.0 ? s_lo + (double)k : s_hi - (double)k;
      // the slab's faces, widened as the boxes of ray_box are (its voxels' corners are sv L, their leaves end at
      // most 66 h above sv L + L), entry face first
      const double base = sv * L, dl = 0x1p-45 * (fabs(base) + L);
      const double f_lo = base - dl, f_hi = (base + L) + dl;
      const double te = ((dm > 0.0 ? f_lo : f_hi) - om) * im, tx = ((dm > 0.0 ? f_hi : f_lo) - om) * im;
      // (no leaf of this slab or of a later one is entered before te: ray_axis's monotonicity)
      if (te > best.t) break;
      const double ta = fmax(te, r.t_min), tb = fmin(tx, r.t_max);
      if (!(ta <= tb)) continue;
      double lo[3], hi[3];
      bool any = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        RAY_RANGE(a, ta, tb, lo[a], hi[a]);
        if (a == m) lo[a] = hi[a] = sv;  // (inside the window: s_lo and s_hi are)
        any = any && lo[a] <= hi[a];
      }
      if (!any) continue;
      // (a slab is 1 voxel thick and |d| <= |d_major|: at most 3 voxels per other axis; bounded whatever happened)
      const int64_t x0 = (int64_t)lo[0], x1 = (int64_t)fmin(hi[0], lo[0] + 7.0);
      const int64_t y0 = (int64_t)lo[1], y1 = (int64_t)fmin(hi[1], lo[1] + 7.0);
      const int64_t z0 = (int64_t)lo[2], z1 = (int64_t)fmin(hi[2], lo[2] + 7.0);
      for (int64_t vx = x0; vx <= x1; ++vx) {
        for (int64_t vy = y0; vy <= y1; ++vy) {
          // (z is the lowest field of the key: the voxels of one column are consecutive codes)
          const uint64_t code1 = vkey_pack(vx, vy, z1, t.org);
          for (int64_t rr = lower_bound_u64(t.vcode, t.V, vkey_pack(vx, vy, z0, t.org)); rr < t.V; ++rr) {
            if (t.vcode[rr] > code1) break;
            ray_walk<PLANE>(T, r, mask, (int32_t)rr, steps, best);
          }
        }
      }
    }
  }
  return best;
}

// ---- every crossed leaf: the walk of octl_forest_ray_evidence (evidence.hip states the definition) ------------------
// Its own march and descent.  They were first written as one template on a leaf visitor with ray_cast as a use; that
// cost k_raycast<true> 16 VGPRs and a wave of occupancy, so ray_cast stays as it is and the two walks
// share Ray, ray_axis, ray_box and RAY_RANGE.
struct EvidenceTables {
  QueryTables t;
  const int32_t* parent;
  int64_t max_steps;
  uint32_t* through;  // [n_nodes] counters the walk adds into
  uint32_t* hits;
};

// F = [t_min, t_free], E = [e0, t_end]; the walk's interval is [t_min, max(t_free, t_end)] (r.t_min, r.t_max)
struct RayIntervals {
  double e0, t_free, t_end;
};

// One ray adds 1 to hits[leaf] of every leaf with in_E, and to through[leaf] of every leaf with in_F and not in_E.  A
// leaf comes here with t_in = max(near, t_min) and t_out = min(far, max(t_free, t_end)) (ray_box with w = 0), and as
// t_min <= e0 and t_free, t_end <= the walk's end,
//   max(near, e0) = max(t_in, e0),  min(far, t_end) = min(t_out, t_end),  min(far, t_free) = min(t_out, t_free):
// the definition's two comparisons on the definition's bits.  An empty F or E fails its comparison by itself
// (t_free < t_min <= max(..); t_end < e0 <= max(..)).
__host__ __device__ __forceinline__ void evidence_leaf(const EvidenceTables& T, const RayIntervals& iv, int32_t node,
                                                       double t_in, double t_out) {
  const bool in_e = fmax(t_in, iv.e0) <= fmin(t_out, iv.t_end);
  const bool in_f = t_in <= fmin(t_out, iv.t_free);
  if (!(in_e || in_f)) return;
  uint32_t* counter = (in_e ? T.hits : T.through) + node;
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(counter, 1u);  // (u32: the sums do not depend on the order of the rays)
#else
  ++*counter;
#endif
}

// The tree under `root` in the order of ray_walk, nothing pruned by a best t: every leaf under `root` that the walk's
// interval crosses is handed to evidence_leaf (a box that contains a crossed leaf is crossed: ray_box), and as the
// order (child number XOR mask) is a permutation of the eight children and the walk only moves to the next sibling
// or up, each at most once.
__host__ __device__ __forceinline__ void evidence_walk(const EvidenceTables& T, const Ray& r, const RayIntervals& iv,
                                                       int mask, int32_t root, int64_t& steps) {
  const QueryTables& t = T.t;
  int32_t node = root;
  for (;;) {
    if (++steps > T.max_steps) return;
    const double cx = t.corner[3 * (int64_t)node + 0], cy = t.corner[3 * (int64_t)node + 1],
                 cz = t.corner[3 * (int64_t)node + 2], e = t.edge[node];
    const int32_t fc = t.first_child[node];
    double t_in, t_out;
    if (ray_box(r, cx, cy, cz, e, fc < 0, t_in, t_out)) {
      if (fc >= 0) {
        node = fc + mask;
        continue;
      }
      evidence_leaf(T, iv, node, t_in, t_out);
    }
    for (;;) {
      if (node == root) return;
      const int32_t par = T.parent[node];
      if (par < 0 || ++steps > T.max_steps) return;
      const int32_t fcp = t.first_child[par];
      const int rank = (node - fcp) ^ mask;
      if (rank >= 0 && rank < 7) {
        node = fcp + ((rank + 1) ^ mask);
        break;
      }
      node = par;
    }
  }
}

// The evidence of one ray.  A dead ray (a value that is not finite, a component with |d| > 1, no axis that bounds
// anything), one whose two intervals are both empty and - in grid mode - one above the cap add nothing.
//
// Every leaf at most ONCE per ray, or it would count double: the march is ray_cast's, and its slabs are one voxel
// thick along the major axis m - lo[m] = hi[m] = sv, and sv differs from slab to slab - while the three loops of a
// slab enumerate distinct (vx, vy, vz).  So no voxel is looked up twice, a voxel has one root (the keys are distinct),
// and evidence_walk hands a leaf under a root over at most once.  (A leaf on a voxel wall that the ray runs along
// belongs to ONE voxel, however many slabs and ranges the wall touches.)
__host__ __device__ __forceinline__ void ray_evidence(const EvidenceTables& T, const double* __restrict__ o,
                                                      const double* __restrict__ d, double t_min, double t_free,
                                                      double t_end) {
  const double INF = HUGE_VAL;
  const QueryTables& t = T.t;
  Ray r;
  r.ox = o[0], r.oy = o[1], r.oz = o[2];
  r.dx = d[0], r.dy = d[1], r.dz = d[2];
  r.t_min = t_min, r.t_max = fmax(t_free, t_end);
  r.ix = 1.0 / r.dx, r.iy = 1.0 / r.dy, r.iz = 1.0 / r.dz;
  r.zx = r.dx == 0.0 || !(fabs(r.ix) < INF);
  r.zy = r.dy == 0.0 || !(fabs(r.iy) < INF);
  r.zz = r.dz == 0.0 || !(fabs(r.iz) < INF);
  const RayIntervals iv = {fmax(t_min, t_free), t_free, t_end};
  // (every comparison is false for NaN; fmax drops one, so t_free and t_end are tested one by one)
  bool live = fabs(r.ox) < INF && fabs(r.oy) < INF && fabs(r.oz) < INF && fabs(r.dx) <= 1.0 && fabs(r.dy) <= 1.0 &&
              fabs(r.dz) <= 1.0 && fabs(t_min) < INF && fabs(t_free) < INF && fabs(t_end) < INF &&
              r.t_min <= r.t_max && !(r.zx && r.zy && r.zz) && t.V > 0;
  const int mask = (r.dx < 0.0 ? 4 : 0) | (r.dy < 0.0 ? 2 : 0) | (r.dz < 0.0 ? 1 : 0);
  int64_t steps = 0;
  if (live && t.mode != 0) {
    evidence_walk(T, r, iv, mask, 0, steps);
  } else if (live && r.t_max - r.t_min <= RAY_CAP_EDGES * t.L && fabs(r.t_min) <= RAY_T_LIMIT * t.L &&
             fabs(r.t_max) <= RAY_T_LIMIT * t.L) {
    // (a ray above the cap is refused by the host form; here it adds nothing)
    const double L = t.L;
    const double adx = fabs(r.dx), ady = fabs(r.dy), adz = fabs(r.dz);
    const int m = (adx >= ady && adx >= adz) ? 0 : (ady >= adz ? 1 : 2);
    const double om = m == 0 ? r.ox : m == 1 ? r.oy : r.oz, dm = m == 0 ? r.dx : m == 1 ? r.dy : r.dz;
    const double im = m == 0 ? r.ix : m == 1 ? r.iy : r.iz;
    const double o3[3] = {r.ox, r.oy, r.oz}, d3[3] = {r.dx, r.dy, r.dz};
    const int32_t g3[3] = {t.org.x, t.org.y, t.org.z};
    double wmin[3], wmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      wmin[a] = fmax(-(double)OCTL_VOX_ABS_LIMIT + 1.0, (double)g3[a] - (double)OCTL_VOX_BIAS + 1.0);
      wmax[a] = fmin((double)OCTL_VOX_ABS_LIMIT - 1.0, (double)g3[a] + (double)OCTL_VOX_BIAS - 1.0);
    }
    double s_lo, s_hi;
    {
      double f0[3], f1[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) RAY_RANGE(a, r.t_min, r.t_max, f0[a], f1[a]);
      s_lo = m == 0 ? f0[0] : m == 1 ? f0[1] : f0[2];
      s_hi = m == 0 ? f1[0] : m == 1 ? f1[1] : f1[2];
    }
    // (at most 256 + 3 slabs; the bound guards the loop whatever the arithmetic did)
    const int64_t n_slabs = s_lo <= s_hi ? (int64_t)fmin(s_hi - s_lo + 1.0, RAY_CAP_EDGES + 8.0) : 0;
    for (int64_t k = 0; k < n_slabs; ++k) {
      const double sv = s_lo + (double)k;  // (any order: nothing ends the march early)
      const double base = sv * L, dl = 0x1p-45 * (fabs(base) + L);
      const double f_lo = base - dl, f_hi = (base + L) + dl;
      const double te = ((dm > 0.0 ? f_lo : f_hi) - om) * im, tx = ((dm > 0.0 ? f_hi : f_lo) - om) * im;
      const double ta = fmax(te, r.t_min), tb = fmin(tx, r.t_max);
      if (!(ta <= tb)) continue;
      double lo[3], hi[3];
      bool any = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        RAY_RANGE(a, ta, tb, lo[a], hi[a]);
        if (a == m) lo[a] = hi[a] = sv;
        any = any && lo[a] <= hi[a];
      }
      if (!any) continue;
      const int64_t x0 = (int64_t)lo[0], x1 = (int64_t)fmin(hi[0], lo[0] + 7.0);
      const int64_t y0 = (int64_t)lo[1], y1 = (int64_t)fmin(hi[1], lo[1] + 7.0);
      const int64_t z0 = (int64_t)lo[2], z1 = (int64_t)fmin(hi[2], lo[2] + 7.0);
      for (int64_t vx = x0; vx <= x1; ++vx) {
        for (int64_t vy = y0; vy <= y1; ++vy) {
          const uint64_t code1 = vkey_pack(vx, vy, z1, t.org);
          for (int64_t rr = lower_bound_u64(t.vcode, t.V, vkey_pack(vx, vy, z0, t.org)); rr < t.V; ++rr) {
            if (t.vcode[rr] > code1) break;
            evidence_walk(T, r, iv, mask, (int32_t)rr, steps);
          }
        }
      }
    }
  }
}
#undef RAY_RANGE
