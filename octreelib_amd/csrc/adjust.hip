// Multi-pose plane adjustment, the device's share: for one rigid transform PER selected pose the block-diagonal
// point-to-plane system of every pose against the leaf planes pooled AT those transforms
// (octl_forest_adjustment_system).  The 6x6 solves, the pose updates and the iteration stay on the host
// (octreelib_amd/adjustment.py: adjustment_system_np is the definition).  No reference counterpart.
//
// No point is read per call.  Under x -> R x + t the moments of a (leaf, pose) block about the leaf's centre a,
// (n, s = sum d, M = sum d d^T, d = x - a), move in closed form (adj_move):
//   a' = ((R_i0 a_x + R_i1 a_y) + R_i2 a_z) + t_i  (transform_np's bits, no fma),  delta = a' - a,
//   s' = R s,  M' = (R M) R^T,  s'' = s' + n delta,  M'' = M' + delta s'^T + s' delta^T + n delta delta^T,
// every dot product as fma(x2, y2, fma(x1, y1, x0 y0)); at R = I, t = 0 every step is exact.
//
// Prepared once per map and pose selection (adj_prepare; stamped as every derived map table is, forest.h):
//   k_adj_hist                              selected blocks per pose (integer atomics)
//   k_pool_keys, sort, k_pool_heads, scan   the (node, slot) grouping of the selected blocks (leaf_moments.h: block_groups)
//   k_adj_moments   one wave per selected block: its 80-byte moments by the chunked reduction of k_pool_moments
//                   (chunk_sums over chunks of 4096, folded in chunk order), its leaf row, its pose
//   k_adj_keys2, sort                       the same blocks by (slot, node); a pose's blocks are one run of it, cut
//                                           into chunks of 1024 blocks that never straddle a pose
// Per call, three launches in stream order and ONE host wait (the download of S x 240 + 8 bytes):
//   k_adj_leaf      one lane per leaf: its blocks in slot order, moved and pooled as k_pool_moments pools them (the
//                   first taken as it is, the later ones added), finish, sym3_eigen, the gates, one 64-byte plane row
//   k_adj_partial   one workgroup of 256 per chunk: lane tid takes blocks j * 256 + tid, j = 0..3 in that order, forms
//                   the block's 28 terms from (n, s'', M'') and the plane (adj_term) - blocks of unused leaves are
//                   skipped by a branch - then the wave butterfly and the wave-order fold of k_reg_partial (sums28.h)
//   k_adj_fold      one workgroup per selected pose: thread k adds the pose's rows k, k + 256, ... in ascending order,
//                   then the same tree; one more workgroup adds k_adj_leaf's per-wave counts of used leaves
// The tree of a pose depends on that pose's selected-block count alone: a term passes through at most
// D = 4 + 6 + 3 + ceil(ceil(nb / 1024) / 256) + 6 + 3 additions.  No floating-point atomics, nothing sized by the CU
// count.  LDS: 960 bytes (k_adj_partial, k_adj_fold).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "leaf_moments.h"
#include "sums28.h"
#include "sym3_eigen.h"

namespace {

constexpr int AJ_CHUNK = 1024;  // blocks per chunk of k_adj_partial
constexpr int AJ_MOM = 10;      // doubles per block: n, sum d (3), sum d d^T (6: xx xy xz yy yz zz)
constexpr int AJ_OUT = 30;      // doubles per result row: the 28 sums, the two counts (int64 bits)

struct AdjParams {
  double c[3];          // origin of the rotational part
  double max_variance;  // < 0: no gate
  int32_t min_points, min_poses;
};

struct AdjMoved {
  double n, s[3], M[6];
};

__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return fma(x2, y2, fma(x1, y1, x0 * y0));
}

// (n, s'', M'') of a block's moments `mom` about the anchor a under T = (R | t), still about a
__device__ __forceinline__ void adj_move(const double* __restrict__ mom, const double* __restrict__ T, double ax,
                                         double ay, double az, AdjMoved& o) {
  const double n = mom[0];
  double d[3], s[3], W[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* R = T + 4 * i;
    d[i] = (((R[0] * ax + R[1] * ay) + R[2] * az) + R[3]) - (i == 0 ? ax : i == 1 ? ay : az);
    s[i] = dot3(R[0], R[1], R[2], mom[1], mom[2], mom[3]);
    W[i][0] = dot3(R[0], R[1], R[2], mom[4], mom[5], mom[6]);
    W[i][1] = dot3(R[0], R[1], R[2], mom[5], mom[7], mom[8]);
    W[i][2] = dot3(R[0], R[1], R[2], mom[6], mom[8], mom[9]);
  }
  o.n = n;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.s[i] = fma(n, d[i], s[i]);
#pragma unroll
    for (int j = i; j < 3; ++j, ++k) {
      const double* Rj = T + 4 * j;
      const double m = dot3(W[i][0], W[i][1], W[i][2], Rj[0], Rj[1], Rj[2]);
      o.M[k] = fma(n * d[i], d[j], fma(s[i], d[j], fma(d[i], s[j], m)));
    }
  }
}

// v x w
__device__ __forceinline__ void cross3(const double* v, const double* w, double* o) {
  o[0] = fma(v[1], w[2], -(v[2] * w[1]));
  o[1] = fma(v[2], w[0], -(v[0] * w[2]));
  o[2] = fma(v[0], w[1], -(v[1] * w[0]));
}

// the 28 terms of one block: with x = a + d, r = nrm . (x - m) = nrm . d + rho and J = [(d + e) x nrm, nrm], e = a - c,
//   H = sum J J^T, g = sum J r, cost = sum r^2 / 2 over the block's points, written in (n, s, M)
__device__ __forceinline__ void adj_term(const AdjMoved& q, const double* nrm, const double* mean, const double* a,
                                         const double* c, double* t) {
  const double e[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
  const double rho = dot3(nrm[0], nrm[1], nrm[2], a[0] - mean[0], a[1] - mean[1], a[2] - mean[2]);
  const double n = q.n;
  const double* M = q.M;
  double k[3], w[3], Mn[3], gm[3], Y[3][3], col[3], G[3];
  cross3(e, nrm, k);    // the constant part of the rotational Jacobian
  cross3(q.s, nrm, w);  // sum d x nrm
  Mn[0] = dot3(M[0], M[1], M[2], nrm[0], nrm[1], nrm[2]);
  Mn[1] = dot3(M[1], M[3], M[4], nrm[0], nrm[1], nrm[2]);
  Mn[2] = dot3(M[2], M[4], M[5], nrm[0], nrm[1], nrm[2]);
  const double ns = dot3(nrm[0], nrm[1], nrm[2], q.s[0], q.s[1], q.s[2]);
  const double nMn = dot3(nrm[0], nrm[1], nrm[2], Mn[0], Mn[1], Mn[2]);
  const double sig = fma(n, rho, ns);  // sum r
  // sum (d x nrm)(d x nrm)^T = K M K^T, K v = v x nrm: rows of M first, then the columns of the result
  const double r0[3] = {M[0], M[1], M[2]}, r1[3] = {M[1], M[3], M[4]}, r2[3] = {M[2], M[4], M[5]};
  cross3(r0, nrm, Y[0]);
  cross3(r1, nrm, Y[1]);
  cross3(r2, nrm, Y[2]);
  const int rr[3] = {0, 6, 11};  // start of rows 0..2 in the packed upper triangle of H
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    col[0] = Y[0][j], col[1] = Y[1][j], col[2] = Y[2][j];
    cross3(col, nrm, G);
#pragma unroll
    for (int i = 0; i <= j; ++i) t[rr[i] + (j - i)] = fma(n * k[i], k[j], fma(k[i], w[j], fma(w[i], k[j], G[i])));
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p = fma(n, k[i], w[i]);  // sum (d + e) x nrm
#pragma unroll
    for (int j = 0; j < 3; ++j) t[rr[i] + (3 - i) + j] = p * nrm[j];
  }
  const double nn[3] = {n * nrm[0], n * nrm[1], n * nrm[2]};
  t[15] = nn[0] * nrm[0], t[16] = nn[0] * nrm[1], t[17] = nn[0] * nrm[2];
  t[18] = nn[1] * nrm[1], t[19] = nn[1] * nrm[2];
  t[20] = nn[2] * nrm[2];
  cross3(Mn, nrm, gm);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[21 + i] = fma(k[i], sig, fma(rho, w[i], gm[i]));
    t[24 + i] = nrm[i] * sig;
  }
  t[27] = 0.5 * fma(n * rho, rho, fma(2.0 * rho, ns, nMn));
}

// ---- preparation --------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_adj_hist(const int32_t* __restrict__ blk_slot, int64_t nb,
                                                  const int32_t* __restrict__ slot_idx, int n_poses,
                                                  uint32_t* __restrict__ hist) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const int32_t s = blk_slot[b];
  if (s < 0 || s >= n_poses) return;
  const int32_t p = slot_idx[s];
  if (p >= 0) atomicAdd(&hist[p], 1u);
}

// one wave per selected block, in (node, slot) order
__global__ __launch_bounds__(256) void k_adj_moments(
    const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, const uint32_t* __restrict__ row_of,
    int64_t n_sel, int sbits, const uint32_t* __restrict__ blk_start, const int32_t* __restrict__ blk_size,
    const double* __restrict__ xyz, const double* __restrict__ corner, const double* __restrict__ edge,
    const int32_t* __restrict__ slot_idx, int n_poses, int64_t n_rows, double* __restrict__ mom,
    int32_t* __restrict__ blk_row, int32_t* __restrict__ blk_pose, int32_t* __restrict__ leaf_first,
    int32_t* __restrict__ leaf_node, double* __restrict__ leaf_anchor) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_sel) return;
  const int lane = threadIdx.x & 63;
  const uint64_t k = key[i];
  const uint64_t node = k >> sbits;
  const int32_t slot = (int32_t)(k & ((1ull << sbits) - 1));
  const bool head = i == 0 || (key[i - 1] >> sbits) != node;
  const int64_t row = (int64_t)row_of[i] - (head ? 0 : 1);
  if (row < 0 || row >= n_rows || slot >= n_poses) return;  // (never: the tables are sized from the scan's total)
  const double h = edge[node] / 2.0;
  const double ax = corner[3 * node + 0] + h, ay = corner[3 * node + 1] + h, az = corner[3 * node + 2] + h;
  const uint32_t b = val[i];
  const int64_t s = blk_start[b];
  const int32_t n = blk_size[b];
  Sums B = chunk_sums(xyz, s, min(n, LS_CHUNK), ax, ay, az, lane);
  for (int32_t c0 = LS_CHUNK; c0 < n; c0 += LS_CHUNK)
    fold(B, chunk_sums(xyz, s + c0, min(n - c0, LS_CHUNK), ax, ay, az, lane));
  if (lane != 0) return;
  double* m = mom + AJ_MOM * i;
  m[0] = (double)n;
#pragma unroll
  for (int q = 0; q < 9; ++q) m[1 + q] = B.s[q];
  blk_row[i] = (int32_t)row;
  blk_pose[i] = slot_idx[slot];
  if (head) {
    leaf_first[row] = (int32_t)i;
    leaf_node[row] = (int32_t)node;
    leaf_anchor[3 * row + 0] = ax, leaf_anchor[3 * row + 1] = ay, leaf_anchor[3 * row + 2] = az;
  }
  if (i == 0) leaf_first[n_rows] = (int32_t)n_sel;
}

__global__ __launch_bounds__(256) void k_adj_keys2(const uint64_t* __restrict__ key, int64_t n_sel, int sbits,
                                                   int nbits, uint64_t* __restrict__ key2,
                                                   uint32_t* __restrict__ val2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sel) return;
  const uint64_t k = key[i];
  key2[i] = ((k & ((1ull << sbits) - 1)) << nbits) | (k >> sbits);
  val2[i] = (uint32_t)i;
}

// ---- one call -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_adj_leaf(int64_t n_rows, const int32_t* __restrict__ leaf_first,
                                                  const double* __restrict__ leaf_anchor,
                                                  const double* __restrict__ mom, const int32_t* __restrict__ blk_pose,
                                                  const double* __restrict__ T, AdjParams P,
                                                  double* __restrict__ plane, int32_t* __restrict__ used,
                                                  int32_t* __restrict__ wave_used) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const double ax = leaf_anchor[3 * r + 0], ay = leaf_anchor[3 * r + 1], az = leaf_anchor[3 * r + 2];
  const int32_t i0 = leaf_first[r], i1 = leaf_first[r + 1];
  Sums S;
#pragma unroll
  for (int q = 0; q < 9; ++q) S.s[q] = 0.0;
  int64_t n_all = 0;
  int32_t n_poses = 0;
  for (int32_t i = i0; i < i1; ++i) {
    AdjMoved m;
    adj_move(mom + (int64_t)AJ_MOM * i, T + 12 * blk_pose[i], ax, ay, az, m);
    Sums B;
#pragma unroll
    for (int q = 0; q < 3; ++q) B.s[q] = m.s[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) B.s[3 + q] = m.M[q];
    if (i == i0) S = B; else fold(S, B);
    n_all += (int64_t)m.n;
    n_poses += m.n > 0.0 ? 1 : 0;
  }
  double mean[3], c6[6], w[3], v[9];
  finish(S, n_all, ax, ay, az, mean, c6);
  sym3_eigen(c6, w, v);
  const bool ok = n_all >= P.min_points && n_poses >= P.min_poses && fabs(w[0]) < INFINITY &&
                  !(P.max_variance >= 0.0 && w[0] > P.max_variance);  // (NaN: unused)
  double* p = plane + 8 * r;
  p[0] = v[0], p[1] = v[3], p[2] = v[6];
  p[3] = mean[0], p[4] = mean[1], p[5] = mean[2];
  p[6] = w[0];
  p[7] = (double)n_all;
  used[r] = ok ? 1 : 0;
  // (the lanes past the last row have left: the ballot counts the wave's rows only)
  const int n_ok = __popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0) wave_used[r >> 6] = n_ok;
}

__global__ __launch_bounds__(256) void k_adj_partial(const int4* __restrict__ chunks, const uint32_t* __restrict__ ord2,
                                                     const double* __restrict__ mom,
                                                     const int32_t* __restrict__ blk_row,
                                                     const double* __restrict__ leaf_anchor,
                                                     const double* __restrict__ plane,
                                                     const int32_t* __restrict__ used, const double* __restrict__ T,
                                                     AdjParams P, double* __restrict__ rows) {
  __shared__ double lds[4][RS_SUMS];
  __shared__ long long ldc[4][2];
  RegAcc a;
  reg_zero(a);
  const int4 ck = chunks[blockIdx.x];  // {pose, first block of the (slot, node) order, blocks, -}
  const double* Tp = T + 12 * ck.x;
#pragma unroll 1
  for (int j = threadIdx.x; j < ck.z; j += 256) {  // (at most AJ_CHUNK / 256 = 4 blocks per lane)
    const int64_t i = ord2[(int64_t)ck.y + j];
    const int32_t row = blk_row[i];
    if (!used[row]) continue;
    const double* an = leaf_anchor + 3 * (int64_t)row;
    const double* pl = plane + 8 * (int64_t)row;
    AdjMoved m;
    adj_move(mom + AJ_MOM * i, Tp, an[0], an[1], an[2], m);
    double t[RS_SUMS];
    adj_term(m, pl, pl + 3, an, P.c, t);
#pragma unroll
    for (int k = 0; k < RS_SUMS; ++k) a.s[k] += t[k];
    a.used += (long long)m.n;
    a.located += 1;
  }
  reg_block_reduce(a, lds, ldc);
  double* out = rows + (int64_t)blockIdx.x * RS_ROW;
  if (threadIdx.x < RS_SUMS) out[threadIdx.x] = a.s[0];
  if (threadIdx.x == 0) {
    reinterpret_cast<long long*>(out)[RS_SUMS] = a.used;
    reinterpret_cast<long long*>(out)[RS_SUMS + 1] = a.located;
  }
}

// workgroup p < S: the rows of pose p; workgroup S: the number of used leaves (k_adj_leaf's per-wave counts added) into
// out[S * AJ_OUT]
__global__ __launch_bounds__(256) void k_adj_fold(const double* __restrict__ rows, const int32_t* __restrict__ chunk_off,
                                                  int S, const int32_t* __restrict__ wave_used, int64_t n_waves,
                                                  double* __restrict__ out) {
  __shared__ double lds[4][RS_SUMS];
  __shared__ long long ldc[4][2];
  RegAcc a;
  reg_zero(a);
  const int p = blockIdx.x;
  if (p == S) {
    for (int64_t r = threadIdx.x; r < n_waves; r += 256) a.used += wave_used[r];
  } else {
    for (int64_t r = (int64_t)chunk_off[p] + threadIdx.x; r < chunk_off[p + 1]; r += 256) {
      const double* in = rows + r * RS_ROW;
#pragma unroll
      for (int k = 0; k < RS_SUMS; ++k) a.s[k] += in[k];
      a.used += reinterpret_cast<const long long*>(in)[RS_SUMS];
      a.located += reinterpret_cast<const long long*>(in)[RS_SUMS + 1];
    }
  }
  reg_block_reduce(a, lds, ldc);
  double* o = out + (int64_t)p * AJ_OUT;
  if (p == S) {
    if (threadIdx.x == 0) reinterpret_cast<long long*>(o)[0] = a.used;
    return;
  }
  if (threadIdx.x < RS_SUMS) o[threadIdx.x] = a.s[0];
  if (threadIdx.x == 0) {
    reinterpret_cast<long long*>(o)[RS_SUMS] = a.used;
    reinterpret_cast<long long*>(o)[RS_SUMS + 1] = a.located;
  }
}

// f->adj_tab for n_sel blocks, n_rows leaves, n_chunks chunks, S selected poses
struct AdjTab {
  size_t n_sel, n_rows, n_chunks, S;
  Carve plan;
  Carve::Part<double> mom = plan.add<double>(n_sel * AJ_MOM);
  Carve::Part<int32_t> row = plan.add<int32_t>(n_sel), pose = plan.add<int32_t>(n_sel);
  Carve::Part<uint32_t> ord2 = plan.add<uint32_t>(n_sel);
  Carve::Part<int32_t> first = plan.add<int32_t>(n_rows + 1), node = plan.add<int32_t>(n_rows);
  Carve::Part<double> anchor = plan.add<double>(n_rows * 3);
  Carve::Part<int4> chunks = plan.add<int4>(n_chunks);
  Carve::Part<int32_t> choff = plan.add<int32_t>(S + 1);
  constexpr AdjTab(int64_t blocks, int64_t rows, int64_t n_ck, int s)
      : n_sel((size_t)blocks), n_rows((size_t)rows), n_chunks((size_t)n_ck), S((size_t)s) {}
};
static_assert(AdjTab(100, 10, 3, 2).choff.off == 10752 && AdjTab(100, 10, 3, 2).plan.total == 11008, "AdjTab offsets");

// f->adj_call: [T 12 f64 per pose | plane 8 f64 per leaf | used i32 per leaf | used leaves i32 per wave of k_adj_leaf |
//               partial rows | result]
struct AdjCall {
  size_t n_rows, n_chunks, S;
  Carve plan;
  Carve::Part<double> T = plan.add<double>(S * 12), plane = plan.add<double>(n_rows * 8);
  Carve::Part<int32_t> used = plan.add<int32_t>(n_rows), wused = plan.add<int32_t>((n_rows + 63) / 64);
  Carve::Part<double> rows = plan.add<double>(n_chunks * RS_ROW), out = plan.add<double>(S * AJ_OUT + 1);
  constexpr AdjCall(int64_t rows_, int64_t n_ck, int s) : n_rows((size_t)rows_), n_chunks((size_t)n_ck), S((size_t)s) {}
};
static_assert(AdjCall(100, 3, 2).out.off == 8192 && AdjCall(100, 3, 2).plan.total == 8704, "AdjCall offsets");

int adj_prepare(octl_forest* f, const std::vector<uint8_t>& sel) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const int64_t nb = f->n_blocks;
  const int n_poses = (int)f->pose_off.size() - 1;
  f->adj_stamp = 0;
  f->adj_called = false;
  std::vector<int32_t> slots, slot_idx((size_t)std::max(n_poses, 1), -1);
  for (int s = 0; s < n_poses; ++s)
    if (sel.empty() || sel[s]) {
      slot_idx[s] = (int32_t)slots.size();
      slots.push_back(s);
    }
  const int S = (int)slots.size();
  std::vector<int64_t> chunk_off((size_t)S + 1, 0);
  int64_t n_sel = 0, n_rows = 0;
  if (nb > 0 && S > 0) {
    // f->grp_scratch: the grouping, then [slot -> selection index i32 | scan total u32, blocks per selected pose u32]
    BlockGroups g(f, true);
    const auto sidx_part = g.plan.add<int32_t>((size_t)n_poses);
    const auto misc_part = g.plan.add<uint32_t>((size_t)S + 1);
    const size_t misc_bytes = ((size_t)S + 1) * 4;
    OCTL_TRY(g.prepare(f, sel));
    int32_t* sidx_d = Carve::at(f->grp_scratch, sidx_part);
    uint32_t* misc_d = Carve::at(f->grp_scratch, misc_part);
    HIP_TRY(ctx, hipMemcpyAsync(sidx_d, slot_idx.data(), (size_t)n_poses * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(misc_d, 0, misc_bytes, st));
    {
      KTimer t(ctx, "adj_group");
      OCTL_LAUNCH(k_adj_hist, dim3(grid_for(nb)), dim3(256), 0, st, (const int32_t*)f->blk_slot.as<int32_t>(), nb,
                  (const int32_t*)sidx_d, n_poses, misc_d + 1);
      HIP_TRY(ctx, hipGetLastError());
      OCTL_TRY(block_groups(f, (int)sel.size(), misc_d, g));
    }
    std::vector<uint32_t> misc((size_t)S + 1);
    HIP_TRY(ctx, hipMemcpyAsync(misc.data(), misc_d, misc_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    n_rows = misc[0];
    std::vector<int4> chunks;
    for (int p = 0; p < S; ++p) {
      const int64_t cnt = misc[(size_t)p + 1];
      for (int64_t c0 = 0; c0 < cnt; c0 += AJ_CHUNK)
        chunks.push_back(make_int4(p, (int)(n_sel + c0), (int)std::min<int64_t>(cnt - c0, AJ_CHUNK), 0));
      n_sel += cnt;
      chunk_off[(size_t)p + 1] = (int64_t)chunks.size();
    }
    if (n_sel > nb || n_rows > n_sel)
      return octl_set_error(ctx, OCTL_E_HIP, "adjustment: inconsistent block grouping (%lld of %lld blocks, %lld leaves)",
                            (long long)n_sel, (long long)nb, (long long)n_rows);
    if (n_sel > 0) {
      const int64_t n_chunks = (int64_t)chunks.size();
      const AdjTab lay(n_sel, n_rows, n_chunks, S);
      DevBuf& tb = f->adj_tab;
      OCTL_TRY(devbuf_reserve(ctx, f->adj_tab, lay.plan.total));
      std::vector<int32_t> choff32(chunk_off.begin(), chunk_off.end());
      // (rows, poses, order and leaf ranges start as zeros: a table the kernels below left incomplete names no memory
      //  outside the tables)
      HIP_TRY(ctx, hipMemsetAsync(Carve::at(tb, lay.row), 0, lay.node.off - lay.row.off, st));
      HIP_TRY(ctx, hipMemcpyAsync(Carve::at(tb, lay.chunks), chunks.data(), (size_t)n_chunks * 16,
                                  hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(Carve::at(tb, lay.choff), choff32.data(), ((size_t)S + 1) * 4, hipMemcpyHostToDevice,
                                  st));
      {
        KTimer t(ctx, "adj_moments");
        const NodeTable& nt = f->nodes[f->cur];
        OCTL_LAUNCH(k_adj_moments, dim3((unsigned)ceil_div(n_sel, 4)), dim3(256), 0, st, (const uint64_t*)g.keys[0],
                    (const uint32_t*)g.vals[0], (const uint32_t*)g.heads, n_sel, g.sbits,
                    (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                    (const double*)f->xyz_ord.as<double>(), (const double*)nt.corner.as<double>(),
                    (const double*)nt.edge.as<double>(), (const int32_t*)sidx_d, n_poses, n_rows,
                    Carve::at(tb, lay.mom), Carve::at(tb, lay.row), Carve::at(tb, lay.pose), Carve::at(tb, lay.first),
                    Carve::at(tb, lay.node), Carve::at(tb, lay.anchor));
        HIP_TRY(ctx, hipGetLastError());
      }
      {
        // (the first order's keys are read for the last time here: the second sort takes their buffers over)
        KTimer t(ctx, "adj_order");
        uint64_t* keys2[2] = {g.keys[1], g.keys[0]};
        uint32_t* vals2[2] = {g.vals[1], g.vals[0]};
        OCTL_LAUNCH(k_adj_keys2, dim3(grid_for(n_sel)), dim3(256), 0, st, (const uint64_t*)g.keys[0], n_sel, g.sbits,
                    g.nbits, keys2[0], vals2[0]);
        HIP_TRY(ctx, hipGetLastError());
        int res2 = 0;
        OCTL_TRY(octl_radix_sort_u64_u32(ctx, keys2, vals2, n_sel, g.kbits, f->pl_hist, &res2));
        HIP_TRY(ctx, hipMemcpyAsync(Carve::at(tb, lay.ord2), vals2[res2], (size_t)n_sel * 4, hipMemcpyDeviceToDevice,
                                    st));
      }
      HIP_TRY(ctx, hipStreamSynchronize(st));  // (the uploads above read host arrays that end with this call)
    }
  }
  f->adj_sel = sel;
  f->adj_slots = slots;
  f->adj_chunk_off = chunk_off;
  f->adj_blocks = n_sel;
  f->adj_rows = n_sel > 0 ? n_rows : 0;
  f->adj_stamp = f->content_stamp;
  return OCTL_OK;
}

}  // namespace

extern "C" {

int octl_forest_adjustment_system(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, const double* transforms,
                                  const double origin[3], int32_t min_points, int32_t min_poses, double max_variance,
                                  double* sums, int64_t* counts, int64_t n_leaves[2]) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "adjustment_system before build");
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  const int n_poses = (int)f->pose_off.size() - 1;
  int S = 0;
  for (int s = 0; s < n_poses; ++s) S += (sel.empty() || sel[s]) ? 1 : 0;
  if (!origin || !n_leaves || (S > 0 && (!transforms || !sums || !counts)))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad adjustment_system arguments");
  for (int k = 0; k < 12 * S; ++k)
    if (!std::isfinite(transforms[k]))
      return octl_set_error(ctx, OCTL_E_INVALID, "adjustment_system: the transform of selected pose %d is not finite",
                            k / 12);
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k]))
      return octl_set_error(ctx, OCTL_E_INVALID, "adjustment_system: the origin is not finite");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!(forest_table_valid(f, f->adj_stamp) && f->adj_sel == sel)) OCTL_TRY(adj_prepare(f, sel));
  f->adj_called = false;
  n_leaves[0] = f->adj_rows;
  n_leaves[1] = 0;
  for (int k = 0; k < RS_SUMS * S; ++k) sums[k] = 0.0;
  for (int k = 0; k < 2 * S; ++k) counts[k] = 0;
  if (f->adj_rows == 0) {  // (nothing to reduce: no launch)
    f->adj_called = true;
    return OCTL_OK;
  }
  hipStream_t st = ctx->stream;
  const int64_t n_rows = f->adj_rows, n_chunks = f->adj_chunk_off[(size_t)S];
  const AdjTab tab(f->adj_blocks, n_rows, n_chunks, S);
  const AdjCall lay(n_rows, n_chunks, S);
  OCTL_TRY(devbuf_reserve(ctx, f->adj_call, lay.plan.total));
  DevBuf &tb = f->adj_tab, &cb = f->adj_call;
  AdjParams P;
  std::memcpy(P.c, origin, sizeof P.c);
  P.max_variance = max_variance >= 0.0 ? max_variance : -1.0;
  P.min_points = min_points;
  P.min_poses = min_poses;
  const double *mom = Carve::at(tb, tab.mom), *anchor = Carve::at(tb, tab.anchor);
  const int32_t *blk_row = Carve::at(tb, tab.row), *blk_pose = Carve::at(tb, tab.pose);
  double *T_d = Carve::at(cb, lay.T), *plane_d = Carve::at(cb, lay.plane), *rows_d = Carve::at(cb, lay.rows);
  double* out_d = Carve::at(cb, lay.out);
  int32_t *used_d = Carve::at(cb, lay.used), *wused_d = Carve::at(cb, lay.wused);
  HIP_TRY(ctx, hipMemcpyAsync(T_d, transforms, (size_t)S * 96, hipMemcpyHostToDevice, st));
  {
    KTimer t(ctx, "adj_leaf");
    OCTL_LAUNCH(k_adj_leaf, dim3(grid_for(n_rows)), dim3(256), 0, st, n_rows,
                (const int32_t*)Carve::at(tb, tab.first), anchor, mom, blk_pose, (const double*)T_d, P,
                plane_d, used_d, wused_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  {
    KTimer t(ctx, "adj_partial");
    OCTL_LAUNCH(k_adj_partial, dim3((unsigned)n_chunks), dim3(256), 0, st,
                (const int4*)Carve::at(tb, tab.chunks), (const uint32_t*)Carve::at(tb, tab.ord2), mom, blk_row, anchor,
                (const double*)plane_d, (const int32_t*)used_d, (const double*)T_d, P, rows_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  {
    KTimer t(ctx, "adj_fold");
    OCTL_LAUNCH(k_adj_fold, dim3((unsigned)S + 1), dim3(256), 0, st, (const double*)rows_d,
                (const int32_t*)Carve::at(tb, tab.choff), S, (const int32_t*)wused_d, ceil_div(n_rows, 64),
                out_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  std::vector<double> out((size_t)S * AJ_OUT + 1);
  HIP_TRY(ctx, hipMemcpyAsync(out.data(), out_d, out.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int p = 0; p < S; ++p) {
    std::memcpy(sums + (size_t)p * RS_SUMS, &out[(size_t)p * AJ_OUT], RS_SUMS * 8);
    std::memcpy(counts + 2 * (size_t)p, &out[(size_t)p * AJ_OUT + RS_SUMS], 16);
  }
  std::memcpy(&n_leaves[1], &out[(size_t)S * AJ_OUT], 8);
  f->adj_called = true;
  return OCTL_OK;
}

int octl_forest_adjustment_tables(octl_forest* f, int64_t cap_leaves, int32_t* node, int64_t* count, double* mean,
                                  double* normal, double* lambda0, uint8_t* used, int64_t* n_leaves,
                                  int64_t cap_blocks, int32_t* blk_node, int32_t* blk_slot, double* blk_moments,
                                  int64_t* n_blocks) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "adjustment_tables before build");
  if (!(forest_table_valid(f, f->adj_stamp) && f->adj_called))
    return octl_set_error(ctx, OCTL_E_STATE,
                          "adjustment_tables: no octl_forest_adjustment_system call on the forest as it is now");
  if (!n_leaves || !n_blocks) return octl_set_error(ctx, OCTL_E_INVALID, "bad adjustment_tables arguments");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int64_t n_rows = f->adj_rows, nb = f->adj_blocks;
  *n_leaves = n_rows;
  *n_blocks = nb;
  if (n_rows == 0) return OCTL_OK;
  const int S = (int)f->adj_slots.size();
  const AdjTab tab(nb, n_rows, f->adj_chunk_off[(size_t)S], S);
  const AdjCall lay(n_rows, f->adj_chunk_off[(size_t)S], S);
  DevBuf &tb = f->adj_tab, &cb = f->adj_call;
  hipStream_t st = ctx->stream;
  const bool leaves = cap_leaves >= n_rows && (node || count || mean || normal || lambda0 || used);
  const bool blocks = cap_blocks >= nb && (blk_node || blk_slot || blk_moments);
  if (!leaves && !blocks) return OCTL_OK;
  std::vector<int32_t> node_h((size_t)n_rows), used_h, row_h, pose_h;
  std::vector<double> plane_h;
  HIP_TRY(ctx, hipMemcpyAsync(node_h.data(), Carve::at(tb, tab.node), (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
  if (leaves) {
    used_h.resize((size_t)n_rows);
    plane_h.resize((size_t)n_rows * 8);
    HIP_TRY(ctx, hipMemcpyAsync(used_h.data(), Carve::at(cb, lay.used), (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(plane_h.data(), Carve::at(cb, lay.plane), (size_t)n_rows * 64, hipMemcpyDeviceToHost, st));
  }
  if (blocks) {
    row_h.resize((size_t)nb);
    pose_h.resize((size_t)nb);
    HIP_TRY(ctx, hipMemcpyAsync(row_h.data(), Carve::at(tb, tab.row), (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(pose_h.data(), Carve::at(tb, tab.pose), (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    if (blk_moments)
      HIP_TRY(ctx, hipMemcpyAsync(blk_moments, Carve::at(tb, tab.mom), (size_t)nb * AJ_MOM * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (leaves)
    for (int64_t r = 0; r < n_rows; ++r) {
      const double* p = &plane_h[(size_t)r * 8];
      if (node) node[r] = node_h[(size_t)r];
      if (count) count[r] = (int64_t)p[7];
      if (normal) std::memcpy(normal + 3 * r, p, 24);
      if (mean) std::memcpy(mean + 3 * r, p + 3, 24);
      if (lambda0) lambda0[r] = p[6];
      if (used) used[r] = used_h[(size_t)r] ? 1 : 0;
    }
  if (blocks)
    for (int64_t i = 0; i < nb; ++i) {
      const int32_t row = row_h[(size_t)i], p = pose_h[(size_t)i];
      if (blk_node) blk_node[i] = row >= 0 && row < n_rows ? node_h[(size_t)row] : -1;
      if (blk_slot) blk_slot[i] = p >= 0 && p < S ? f->adj_slots[(size_t)p] : -1;
    }
  return OCTL_OK;
}

}  // extern "C"
