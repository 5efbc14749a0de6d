// Plane segments: the leaves of the pooled plane table merged across their faces into connected coplanar regions
// (octl_forest_plane_segments).  Defined by octreelib_amd/query.py: plane_segments_np - neighbour,
// label, root and leaf count equal it exactly, the merged moments within the bound stated there.  No reference
// counterpart: the reference has no query across leaves.
//
// Every decision is made on the bits of the pooled table with separate products and sums (-ffp-contract=off):
//   eligible   count >= min_points, lambda0 finite, lambda0 <= max_variance when one is given;
//   neighbour  locate_one of the leaf's centre with one coordinate moved onto the + face (c + e: cubes are half-open)
//              or just below the - face (the double before c), -1 for no leaf or the leaf itself;
//   edge       both rows eligible, |(ni.x nj.x + ni.y nj.y) + ni.z nj.z| >= cos_min, and |n . (mj - mi)| <= max_offset
//              for n = ni and n = nj, the difference rounded once per component.
//
// Launches of a computation (stream order; one readback of two words - segments, error word - then the downloads):
//   k_seg_init     one lane per row: parent[i] = i for an eligible row, -1 otherwise
//   k_seg_link     one lane per (row, direction): probe, walk, gate, lock-free union of the two rows
//   k_seg_flatten  one lane per row: its root, head flag where root == row
//   [scan]         exclusive scan of the head flags: the compact number of every root
//   k_seg_keys     one lane per row: label, sort key = segment (a row without a segment behind all), value = row
//   [radix sort]   stable, so a segment becomes one run in ascending row order - the order segment << 32 | row
//                  would give, in ceil(bits(segments) / 8) passes instead of four more
//   k_seg_starts   one lane per sorted position: first position of every segment
//   k_seg_merge    one wave per segment: moments of the run, 64-lane butterfly, mean, covariance, eigen step
//
// Why the labels are a function of the input: a union hooks the LARGER of two roots under the smaller with a 32-bit
// compare-and-swap that succeeds only while the larger one still is a root.  parent[x] <= x therefore holds at every
// moment - no cycle can form - every successful hook joins exactly two trees that an edge connects, and an edge's lane
// retires only when both ends have one root.  When the kernel ends the trees are the connected components, and the
// root of a tree, having no smaller parent, is its smallest row, whatever the order in which the lanes ran.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "leaf_moments.h"
#include "query_walk.h"
#include "sym3_eigen.h"
#include "union_find.h"

namespace {

struct SegGate {
  int32_t min_points;
  double max_variance;  // < 0: no variance test
  double cos_min, max_offset;
};

// words of the scalar part of f->seg_sort
enum { SEG_W_TOTAL = 0, SEG_W_ERR = 1 };

__device__ __forceinline__ bool seg_eligible(const double2* __restrict__ rows, int64_t row, const SegGate& g) {
  const double2 w = rows[4 * row + 3];  // {lambda0, count}
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  return w.y >= (double)g.min_points && fabs(w.x) < INF && !(g.max_variance >= 0.0 && w.x > g.max_variance);
}

// the double before c (nextafter(c, -inf) for finite c; below +-0 the smallest negative subnormal)
__device__ __forceinline__ double seg_before(double c) {
  if (c == 0.0) return __longlong_as_double((long long)0x8000000000000001ull);
  const long long b = __double_as_longlong(c);
  return __longlong_as_double(c > 0.0 ? b - 1 : b + 1);
}

__global__ __launch_bounds__(256) void k_seg_init(int64_t n_rows, const double2* __restrict__ rows, SegGate g,
                                                  int32_t* __restrict__ parent, uint32_t* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) words[SEG_W_ERR] = 0;
  if (i >= n_rows) return;
  parent[i] = seg_eligible(rows, i, g) ? (int32_t)i : -1;
}

__global__ __launch_bounds__(256) void k_seg_link(int64_t n_rows, const int32_t* __restrict__ row_node, QueryTables t,
                                                  PlaneTable pt, SegGate g, int64_t n_nodes, int64_t max_steps,
                                                  int32_t* __restrict__ neighbour, int32_t* parent,
                                                  uint32_t* __restrict__ words) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= 6 * n_rows) return;
  const int64_t i = tid / 6;
  const int dir = (int)(tid - 6 * i);
  const int axis = dir >> 1;
  const int32_t node = row_node[i];
  int32_t nb = -1;
  if (node >= 0 && node < n_nodes) {
    const double e = t.edge[node];
    const double h = e / 2.0;
    double c[3], p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = t.corner[3 * (int64_t)node + a];
      p[a] = c[a] + h;
    }
    const double moved = (dir & 1) ? c[axis] + e : seg_before(c[axis]);
    p[0] = axis == 0 ? moved : p[0];
    p[1] = axis == 1 ? moved : p[1];
    p[2] = axis == 2 ? moved : p[2];
    nb = locate_one(t, p[0], p[1], p[2]);
    if (nb == node || nb >= n_nodes) nb = -1;
  }
  neighbour[tid] = nb;
  if (nb < 0) return;
  const int32_t j = pt.node_row[nb];
  if (j < 0 || j >= n_rows || j == i) return;
  if (!seg_eligible(pt.rows, i, g) || !seg_eligible(pt.rows, j, g)) return;
  const double2 *ri = pt.rows + 4 * i, *rj = pt.rows + 4 * (int64_t)j;
  const double2 a0 = ri[0], a1 = ri[1], a2 = ri[2], b0 = rj[0], b1 = rj[1], b2 = rj[2];
  // {nx, ny}, {nz, mx}, {my, mz}
  const double dot = (a0.x * b0.x + a0.y * b0.y) + a1.x * b1.x;
  if (!(fabs(dot) >= g.cos_min)) return;
  const double dx = b1.y - a1.y, dy = b2.x - a2.x, dz = b2.y - a2.y;
  const double oi = (a0.x * dx + a0.y * dy) + a1.x * dz;
  const double oj = (b0.x * dx + b0.y * dy) + b1.x * dz;
  if (!(fabs(oi) <= g.max_offset && fabs(oj) <= g.max_offset)) return;
  // ---- union of rows i and j (union_find.h) ----
  int64_t budget = max_steps;
  if (uf_union(parent, (int32_t)i, j, budget) < 0) atomicOr(words + SEG_W_ERR, 1u);
}

__global__ __launch_bounds__(256) void k_seg_flatten(int64_t n_rows, int64_t max_steps, int32_t* parent,
                                                     int32_t* __restrict__ root, uint32_t* __restrict__ heads,
                                                     uint32_t* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  int32_t r = -1;
  if (uf_load(parent + i) >= 0) {
    int64_t budget = max_steps;
    r = uf_find(parent, (int32_t)i, budget);
    if (r < 0) atomicOr(words + SEG_W_ERR, 1u);
  }
  root[i] = r;
  heads[i] = r == (int32_t)i ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_seg_keys(int64_t n_rows, const int32_t* __restrict__ root,
                                                  const uint32_t* __restrict__ number, uint32_t n_segs,
                                                  int32_t* __restrict__ label, uint64_t* __restrict__ key,
                                                  uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int32_t r = root[i];
  const uint32_t s = r >= 0 ? number[r] : n_segs;  // (no segment: behind every segment)
  label[i] = r >= 0 ? (int32_t)s : -1;
  key[i] = (uint64_t)s;
  val[i] = (uint32_t)i;
}

// first[s] = the first sorted position of segment s, first[n_segs] = the end of the last one
__global__ __launch_bounds__(256) void k_seg_starts(const uint64_t* __restrict__ key, int64_t n_rows, uint32_t n_segs,
                                                    uint32_t* __restrict__ first) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_rows) return;
  const uint64_t s = key[p];
  if (s <= n_segs && (p == 0 || key[p - 1] != s)) first[s] = (uint32_t)p;
  if (p == n_rows - 1 && s < n_segs) first[n_segs] = (uint32_t)n_rows;
}

struct SegOut {
  int32_t* root;
  int32_t* n_leaves;
  int64_t* count;
  double* mean;
  double* cov;
  double* eigval;
  double* eigvec;
};

// One wave per segment.  With anchor a = the mean of the segment's smallest row, d = m - a and n, C the count and
// covariance of a row, lane l folds the run's entries l, l + 64, ... in that order,
//   N += n,  S_d += n d (fma),  S_dd += n (C + d d^T) (the term by fma, then fma into the sum),
// the lanes are folded by the butterfly xor 32 .. 1, and lane 0 finishes as a leaf is finished (leaf_moments.h:
// finish) and decomposes the covariance.  The tree of additions depends on the segment's leaf count alone.  A segment
// of one leaf copies the row.
__global__ __launch_bounds__(256) void k_seg_merge(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ first,
                                                   int64_t n_rows, uint32_t n_segs, const int32_t* __restrict__ r_node,
                                                   const int64_t* __restrict__ r_count,
                                                   const double* __restrict__ r_mean, const double* __restrict__ r_cov,
                                                   const double* __restrict__ r_w, const double* __restrict__ r_v,
                                                   SegOut o) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= (int64_t)n_segs) return;
  const int lane = threadIdx.x & 63;
  const int64_t p0 = first[s], p1 = min((int64_t)first[s + 1], n_rows);
  if (p0 >= p1) return;  // (never: every segment holds its root)
  const int64_t r0 = min((int64_t)rows[p0], n_rows - 1);
  if (p1 - p0 == 1) {
    if (lane == 0) {
      o.root[s] = r_node[r0];
      o.n_leaves[s] = 1;
      o.count[s] = r_count[r0];
    }
    if (lane < 3) o.mean[3 * s + lane] = r_mean[3 * r0 + lane];
    if (lane < 6) o.cov[6 * s + lane] = r_cov[6 * r0 + lane];
    if (lane < 3) o.eigval[3 * s + lane] = r_w[3 * r0 + lane];
    if (lane < 9) o.eigvec[9 * s + lane] = r_v[9 * r0 + lane];
    return;
  }
  const double ax = r_mean[3 * r0 + 0], ay = r_mean[3 * r0 + 1], az = r_mean[3 * r0 + 2];
  Sums S;
#pragma unroll
  for (int k = 0; k < 9; ++k) S.s[k] = 0.0;
  long long N = 0;
  for (int64_t p = p0 + lane; p < p1; p += 64) {
    const int64_t r = min((int64_t)rows[p], n_rows - 1);
    const long long cnt = r_count[r];
    const double n = (double)cnt;
    const double dx = r_mean[3 * r + 0] - ax, dy = r_mean[3 * r + 1] - ay, dz = r_mean[3 * r + 2] - az;
    const double* c = r_cov + 6 * r;
    N += cnt;
    S.s[0] = fma(n, dx, S.s[0]);
    S.s[1] = fma(n, dy, S.s[1]);
    S.s[2] = fma(n, dz, S.s[2]);
    S.s[3] = fma(n, fma(dx, dx, c[0]), S.s[3]);
    S.s[4] = fma(n, fma(dx, dy, c[1]), S.s[4]);
    S.s[5] = fma(n, fma(dx, dz, c[2]), S.s[5]);
    S.s[6] = fma(n, fma(dy, dy, c[3]), S.s[6]);
    S.s[7] = fma(n, fma(dy, dz, c[4]), S.s[7]);
    S.s[8] = fma(n, fma(dz, dz, c[5]), S.s[8]);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) S.s[k] += __shfl_xor(S.s[k], m);
    N += __shfl_xor(N, m);
  }
  if (lane == 0) {
    double m3[3], c6[6], w[3], v[9];
    finish(S, (int64_t)N, ax, ay, az, m3, c6);
    sym3_eigen(c6, w, v);
    o.root[s] = r_node[r0];
    o.n_leaves[s] = (int32_t)(p1 - p0);
    o.count[s] = (int64_t)N;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.mean[3 * s + k] = m3[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) o.cov[6 * s + k] = c6[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.eigval[3 * s + k] = w[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o.eigvec[9 * s + k] = v[k];
  }
}

// f->seg_tab for `rows` rows: [neighbour i32 x6 | label i32]
struct SegRowLayout {
  size_t r;  // rows (at least one)
  Carve plan;
  Carve::Part<int32_t> neighbour = plan.add<int32_t>(6 * r), label = plan.add<int32_t>(r);
  constexpr explicit SegRowLayout(int64_t rows) : r((size_t)std::max<int64_t>(rows, 1)) {}
};
static_assert(SegRowLayout(100).label.off == 2560 && SegRowLayout(100).plan.total == 3072, "SegRowLayout offsets");

// f->seg_out for `cap` segments: [root i32 | leaves i32 | count i64 | mean 3 | cov 6 | eigval 3 | eigvec 9]
struct SegOutLayout {
  size_t c;  // segments (at least one)
  Carve plan;
  Carve::Part<int32_t> root = plan.add<int32_t>(c), leaves = plan.add<int32_t>(c);
  Carve::Part<int64_t> count = plan.add<int64_t>(c);
  Carve::Part<double> mean = plan.add<double>(3 * c), cov = plan.add<double>(6 * c), w = plan.add<double>(3 * c),
                      v = plan.add<double>(9 * c);
  constexpr explicit SegOutLayout(int64_t cap) : c((size_t)std::max<int64_t>(cap, 1)) {}
};
static_assert(SegOutLayout(100).v.off == 12032 && SegOutLayout(100).plan.total == 19456, "SegOutLayout offsets");

int segments_compute(octl_forest* f, const QueryTables& qt, const std::vector<uint8_t>& sel, const SegGate& g) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  f->seg_stamp = 0;
  const int64_t R = f->pl_n, n_nodes = f->nodes[f->cur].n;
  int64_t S = 0;
  if (R > 0) {
    const SegRowLayout rl(R);
    OCTL_TRY(devbuf_reserve(ctx, f->seg_tab, rl.plan.total));
    // f->seg_sort: [parent i32 | root i32 | heads u32 (+8: the scan's tail) | key u64 x2 | val u32 x2 |
    //               first u32 (rows + 1) | total, error word]
    Carve plan;
    const size_t r = (size_t)R;
    const auto parent_part = plan.add<int32_t>(r), root_part = plan.add<int32_t>(r);
    const auto heads_part = plan.add<uint32_t>(r + 8);
    const auto key0_part = plan.add<uint64_t>(r), key1_part = plan.add<uint64_t>(r);
    const auto val0_part = plan.add<uint32_t>(r), val1_part = plan.add<uint32_t>(r);
    const auto first_part = plan.add<uint32_t>(r + 1), words_part = plan.add<uint32_t>(2);
    OCTL_TRY(devbuf_reserve(ctx, f->seg_sort, plan.total));
    DevBuf& sb = f->seg_sort;
    int32_t *neighbour = Carve::at(f->seg_tab, rl.neighbour), *label = Carve::at(f->seg_tab, rl.label);
    int32_t *parent = Carve::at(sb, parent_part), *root = Carve::at(sb, root_part);
    uint32_t *heads = Carve::at(sb, heads_part), *first = Carve::at(sb, first_part), *words = Carve::at(sb, words_part);
    uint64_t* keys[2] = {Carve::at(sb, key0_part), Carve::at(sb, key1_part)};
    uint32_t* vals[2] = {Carve::at(sb, val0_part), Carve::at(sb, val1_part)};
    const PoolLayout pl(f->pl_cap);
    const int32_t* r_node = Carve::at(f->pl_rows, pl.node);
    PlaneTable pt;
    pt.node_row = f->pl_node_row.as<int32_t>();
    pt.rows = f->pl_plane.as<double2>();
    pt.min_points = g.min_points;
    pt.max_variance = g.max_variance;
    // more steps than a sound table lets one lane take: a path is shorter than the rows, a union retries only when
    // another lane's hook succeeded
    const int64_t max_steps = 8 * R + 64;
    {
      KTimer t(ctx, "seg_init");
      OCTL_LAUNCH(k_seg_init, dim3(grid_for(R)), dim3(256), 0, st, R, pt.rows, g, parent, words);
      HIP_TRY(ctx, hipGetLastError());
    }
    {
      KTimer t(ctx, "seg_link");
      OCTL_LAUNCH(k_seg_link, dim3(grid_for(6 * R)), dim3(256), 0, st, R, r_node, qt, pt, g, n_nodes, max_steps,
                  neighbour, parent, words);
      HIP_TRY(ctx, hipGetLastError());
    }
    {
      KTimer t(ctx, "seg_flatten");
      OCTL_LAUNCH(k_seg_flatten, dim3(grid_for(R)), dim3(256), 0, st, R, max_steps, parent, root, heads, words);
      HIP_TRY(ctx, hipGetLastError());
    }
    {
      KTimer t(ctx, "seg_scan");
      OCTL_TRY(octl_exclusive_scan_u32(ctx, heads, heads, R, words + SEG_W_TOTAL));
    }
    uint32_t got[2] = {0, 0};
    OCTL_TRY(octl_readback(ctx, words, 2, got));
    if (got[SEG_W_ERR] != 0)
      return octl_set_error(ctx, OCTL_E_STATE,
                            "plane_segments: the union-find ran out of its step budget (a damaged plane table)");
    S = got[SEG_W_TOTAL];
    {
      KTimer t(ctx, "seg_keys");
      OCTL_LAUNCH(k_seg_keys, dim3(grid_for(R)), dim3(256), 0, st, R, (const int32_t*)root, (const uint32_t*)heads,
                  (uint32_t)S, label, keys[0], vals[0]);
      HIP_TRY(ctx, hipGetLastError());
    }
    if (S > 0) {
      const SegOutLayout ol(S);
      OCTL_TRY(devbuf_reserve(ctx, f->seg_out, ol.plan.total));
      DevBuf& ob = f->seg_out;
      const SegOut o{Carve::at(ob, ol.root), Carve::at(ob, ol.leaves), Carve::at(ob, ol.count), Carve::at(ob, ol.mean),
                     Carve::at(ob, ol.cov),  Carve::at(ob, ol.w),      Carve::at(ob, ol.v)};
      int res = 0;
      {
        KTimer t(ctx, "seg_sort");
        OCTL_TRY(octl_radix_sort_u64_u32(ctx, keys, vals, R, std::max(1, bits_for((uint64_t)S)), f->pl_hist, &res));
      }
      KTimer t(ctx, "seg_merge");
      OCTL_LAUNCH(k_seg_starts, dim3(grid_for(R)), dim3(256), 0, st, (const uint64_t*)keys[res], R, (uint32_t)S,
                  first);
      HIP_TRY(ctx, hipGetLastError());
      OCTL_LAUNCH(k_seg_merge, dim3((unsigned)ceil_div(S, 4)), dim3(256), 0, st, (const uint32_t*)vals[res],
                  (const uint32_t*)first, R, (uint32_t)S, r_node, (const int64_t*)Carve::at(f->pl_rows, pl.count),
                  (const double*)Carve::at(f->pl_rows, pl.mean), (const double*)Carve::at(f->pl_rows, pl.cov),
                  (const double*)Carve::at(f->pl_rows, pl.w), (const double*)Carve::at(f->pl_rows, pl.v), o);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  f->seg_rows = R;
  f->seg_n = f->seg_cap = S;
  f->seg_sel = sel;
  f->seg_min_points = g.min_points;
  f->seg_max_variance = g.max_variance;
  f->seg_cos_min = g.cos_min;
  f->seg_max_offset = g.max_offset;
  f->seg_stamp = f->content_stamp;
  return OCTL_OK;
}

}  // namespace

extern "C" int octl_forest_plane_segments(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int32_t min_points,
                                          double max_variance, double cos_min, double max_offset, int64_t cap_rows,
                                          int64_t cap_segments, int32_t* neighbour, int32_t* label, int32_t* root,
                                          int32_t* n_leaves, int64_t* count, double* mean, double* cov6,
                                          double* eigval, double* eigvec, int64_t* n_rows, int64_t* n_segments) {
  if (!f || !n_rows || !n_segments) return OCTL_E_INVALID;
  octl_ctx* ctx = f->ctx;
  // (what is refused whatever the map is refused before anything runs)
  if (min_points < 1) return octl_set_error(ctx, OCTL_E_INVALID, "plane_segments: min_points = %d is below 1", min_points);
  if (!(cos_min >= 0.0 && cos_min <= 1.0))
    return octl_set_error(ctx, OCTL_E_INVALID, "plane_segments: cos_min %g is outside [0, 1] (max_angle in [0, pi/2])",
                          cos_min);
  if (!(std::isfinite(max_offset) && max_offset >= 0.0))
    return octl_set_error(ctx, OCTL_E_INVALID, "plane_segments: max_offset must be finite and not negative");
  if (std::isnan(max_variance)) return octl_set_error(ctx, OCTL_E_INVALID, "plane_segments: max_variance is NaN");
  QueryTables qt;
  OCTL_TRY(query_begin(f, "plane_segments", &qt));
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  SegGate g;
  g.min_points = min_points;
  g.max_variance = max_variance >= 0.0 ? max_variance : -1.0;
  g.cos_min = cos_min;
  g.max_offset = max_offset;
  if (!(forest_table_valid(f, f->pl_stamp) && f->pl_sel == sel)) {
    f->seg_stamp = 0;  // (made from another table)
    OCTL_TRY(pooled_compute(f, sel));
  }
  // (a fill behind a size query finds the tables the query made: the same arguments on an unchanged forest)
  if (!(forest_table_valid(f, f->seg_stamp) && f->seg_sel == sel && f->seg_rows == f->pl_n &&
        f->seg_min_points == g.min_points && f->seg_max_variance == g.max_variance && f->seg_cos_min == g.cos_min &&
        f->seg_max_offset == g.max_offset))
    OCTL_TRY(segments_compute(f, qt, sel, g));
  const int64_t R = f->seg_rows, S = f->seg_n;
  *n_rows = R;
  *n_segments = S;
  if (cap_rows < R || cap_segments < S) return OCTL_OK;
  bool any = false;
  const SegRowLayout rl(R);
  const SegOutLayout ol(f->seg_cap);
  const size_t r = (size_t)R, n = (size_t)S;
  HIP_TRY(ctx, octl_download(ctx, neighbour, f->seg_tab, rl.neighbour, r * 6, &any));
  HIP_TRY(ctx, octl_download(ctx, label, f->seg_tab, rl.label, r, &any));
  HIP_TRY(ctx, octl_download(ctx, root, f->seg_out, ol.root, n, &any));
  HIP_TRY(ctx, octl_download(ctx, n_leaves, f->seg_out, ol.leaves, n, &any));
  HIP_TRY(ctx, octl_download(ctx, count, f->seg_out, ol.count, n, &any));
  HIP_TRY(ctx, octl_download(ctx, mean, f->seg_out, ol.mean, n * 3, &any));
  HIP_TRY(ctx, octl_download(ctx, cov6, f->seg_out, ol.cov, n * 6, &any));
  HIP_TRY(ctx, octl_download(ctx, eigval, f->seg_out, ol.w, n * 3, &any));
  HIP_TRY(ctx, octl_download(ctx, eigvec, f->seg_out, ol.v, n * 9, &any));
  if (any) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OCTL_OK;
}
