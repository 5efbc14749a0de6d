// Planarity statistic of the level loop's fresh nodes (octl_forest_build_planar): for every node created at the
// previous level, the smallest eigenvalue of the covariance of its SCHEME points, which run_level_loop's split
// predicate then compares with max_variance (criteria.py: NotPlanar).
//
// A node's points are the positions [start, start + count) of the level buffer (store index | scheme bit per
// position; the coordinates are gathered through the index).  With the anchor a = corner + edge / 2 (the node's
// centre: exact for the dyadic cubes of the parity domain, and any other anchor would do - the shifted form is exact
// in a) and d = p - a, |d|_inf <= e / 2 (+ one rounding), the moments are
//   S = sum over the node's chunks c = 0, 1, ... (in that order) of P_c,
//   P_c = the reduction of chunk c = positions [c L, min((c+1) L, count)), L = 4096: lane l of a group of G lanes
//         accumulates the scheme points among positions l, l + G, ... of the chunk (sums of d and d d^T, f64, fma),
//         then a butterfly (xor G/2, ..., 1) leaves the totals in every lane of the group;
//   G = 16 for a node of at most 64 positions (four such nodes share a wave), 64 otherwise.
// S is a function of the node's positions alone - not of the launch shape, not of the other nodes of the level - so
// a node's bits are the same in every build that gives it the same point sequence.  Positions that are not scheme
// points are skipped: they add nothing and round nothing.
//
// Error (eps = 2^-53, n scheme points among c positions): a point's contribution passes at most
//   min(n, ceil(min(c, L) / G)) - 1 additions in its lane, log2 G in the butterfly, ceil(c / L) - 1 chunk folds,
// and its products are formed by one fma each, so with gamma = (ceil(c/64) + ceil(c/L) + 16) eps for c > 64
// (for c <= 64: at most 4 + 4 additions, below the 16) every entry of S_dd is within gamma n (e/2)^2 of the exact
// sum and every entry of S_d within gamma n (e/2); the covariance C = S_dd / (n - ddof) - n / (n - ddof) m m^T,
// m = S_d / n, inherits 4 gamma (e/2)^2 n / (n - ddof) per entry (DESIGN 4.6 with R = e / 2), the Jacobi solver adds
// 64 eps ||C||_F.  When every pose drives the scheme c = n and gamma is the bound of DESIGN 4.6.
//
// Launches per level (stream order, no host wait of their own):
//   [fill]          the chunk counter
//   k_node_moments  one wave per four fresh nodes: small nodes in 16-lane groups side by side, nodes of up to L
//                   positions by the whole wave one after the other; a larger node books ceil(c / L) work items
//   k_node_chunks   one wave per work item (grid-stride): P_c of one chunk into the context's scratch
//   k_node_lambda   one lane per fresh node: folds the chunk partials in chunk order, forms C, smallest eigenvalue
// Nodes with fewer than min_points scheme points are skipped; their statistic is NaN.
#include <algorithm>

#include "build_common.h"
#include "common.h"
#include "forest.h"
#include "sym3_eigen.h"

namespace {

constexpr int NM_CHUNK = 64 * 64;  // L: positions per chunk
constexpr int NM_SMALL = 64;       // nodes of at most this many positions are reduced by 16 lanes

struct Sums {
  double s[9];  // sum dx, dy, dz; sum dx dx, dx dy, dx dz, dy dy, dy dz, dz dz
};

__device__ __forceinline__ void zero(Sums& a) {
#pragma unroll
  for (int k = 0; k < 9; ++k) a.s[k] = 0.0;
}

// one position of the level buffer into a lane's sums (nothing for a point that is not a scheme point)
__device__ __forceinline__ void take(Sums& a, uint32_t v, const double* __restrict__ xyz, int xs, double ax,
                                     double ay, double az) {
  if (!(v >> 31)) return;
  const double* p = xyz + (int64_t)xs * (int64_t)(v & IDX_MASK);
  const double dx = p[0] - ax, dy = p[1] - ay, dz = p[2] - az;
  a.s[0] += dx;
  a.s[1] += dy;
  a.s[2] += dz;
  a.s[3] = fma(dx, dx, a.s[3]);
  a.s[4] = fma(dx, dy, a.s[4]);
  a.s[5] = fma(dx, dz, a.s[5]);
  a.s[6] = fma(dy, dy, a.s[6]);
  a.s[7] = fma(dy, dz, a.s[7]);
  a.s[8] = fma(dz, dz, a.s[8]);
}

template <int G>
__device__ __forceinline__ void butterfly(Sums& a) {
#pragma unroll
  for (int m = G / 2; m >= 1; m >>= 1)
#pragma unroll
    for (int k = 0; k < 9; ++k) a.s[k] += __shfl_xor(a.s[k], m);
}

// P_c of positions [first, first + cnt), cnt <= L, over the whole wave; every lane returns it
__device__ __forceinline__ Sums chunk_sums(const uint32_t* __restrict__ idx, uint32_t first, int cnt,
                                           const double* __restrict__ xyz, int xs, double ax, double ay, double az,
                                           int lane) {
  Sums a;
  zero(a);
  for (int j = lane; j < cnt; j += 64) take(a, idx[first + j], xyz, xs, ax, ay, az);
  butterfly<64>(a);
  return a;
}

struct NodeGeom {
  uint32_t start, count;
  double ax, ay, az;
};
__device__ __forceinline__ NodeGeom node_geom(const NodePtrs& nd, int64_t c) {
  NodeGeom g;
  g.start = nd.start[c];
  g.count = nd.count[c];
  const double h = nd.edge[c] * 0.5;
  g.ax = nd.corner[3 * c] + h;
  g.ay = nd.corner[3 * c + 1] + h;
  g.az = nd.corner[3 * c + 2] + h;
  return g;
}

__global__ void k_node_moments(NodePtrs nd, int64_t first, int64_t n_new, int32_t min_points,
                               const uint32_t* __restrict__ idx, const double* __restrict__ xyz, int xs,
                               uint32_t* __restrict__ counter, int2* __restrict__ work, int64_t cap,
                               int32_t* __restrict__ base, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t j0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4;
  if (j0 >= n_new) return;
  // ---- nodes of at most NM_SMALL positions: one 16-lane group each, the four side by side -----------------------
  {
    const int g = lane >> 4, sub = lane & 15;
    const int64_t j = j0 + g;
    Sums a;
    zero(a);
    bool mine = false;
    if (j < n_new && (int64_t)nd.scount[first + j] >= min_points) {
      const NodeGeom ng = node_geom(nd, first + j);
      if (ng.count <= NM_SMALL) {
        mine = true;
        for (uint32_t q = sub; q < ng.count; q += 16) take(a, idx[ng.start + q], xyz, xs, ng.ax, ng.ay, ng.az);
      }
    }
    butterfly<16>(a);
    if (mine && sub == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) sums[9 * j + k] = a.s[k];
      base[j] = -1;
    }
  }
  // ---- the larger ones: the whole wave, one node after the other (all of this is wave-uniform) ------------------
  for (int g = 0; g < 4; ++g) {
    const int64_t j = j0 + g;
    if (j >= n_new) break;
    if ((int64_t)nd.scount[first + j] < min_points) continue;
    const NodeGeom ng = node_geom(nd, first + j);
    if (ng.count <= NM_SMALL) continue;
    if (ng.count <= NM_CHUNK) {
      const Sums S = chunk_sums(idx, ng.start, (int)ng.count, xyz, xs, ng.ax, ng.ay, ng.az, lane);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) sums[9 * j + k] = S.s[k];
        base[j] = -1;
      }
      continue;
    }
    // more than L positions: book the chunks; k_node_chunks reduces them, k_node_lambda folds them
    const int32_t nc = (int32_t)((ng.count + NM_CHUNK - 1) / NM_CHUNK);
    int32_t off = -1;
    if (lane == 0) {
      const uint32_t o = atomicAdd(counter, (uint32_t)nc);
      // (always: the nodes of a level are disjoint runs of n_alive positions, each of them longer than L, so their
      //  chunks number less than 2 n_alive / L)
      off = ((int64_t)o + nc <= cap) ? (int32_t)o : -1;
      base[j] = off >= 0 ? off : -2;
    }
    off = __shfl(off, 0);
    if (off >= 0)
      for (int c = lane; c < nc; c += 64) work[off + c] = make_int2((int32_t)j, c);
  }
}

__global__ void k_node_chunks(const uint32_t* __restrict__ counter, const int2* __restrict__ work, int64_t cap,
                              NodePtrs nd, int64_t first, const uint32_t* __restrict__ idx,
                              const double* __restrict__ xyz, int xs, double* __restrict__ partial) {
  const int64_t total = min((int64_t)*counter, cap);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += waves) {
    const int2 w = work[t];
    const NodeGeom ng = node_geom(nd, first + w.x);
    const uint32_t c0 = (uint32_t)w.y * NM_CHUNK;
    const Sums P = chunk_sums(idx, ng.start + c0, (int)min(ng.count - c0, (uint32_t)NM_CHUNK), xyz, xs, ng.ax, ng.ay,
                              ng.az, lane);
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 9; ++k) partial[9 * t + k] = P.s[k];
  }
}

__global__ void k_node_lambda(NodePtrs nd, int64_t first, int64_t n_new, int32_t min_points, int32_t ddof,
                              const int32_t* __restrict__ base, const double* __restrict__ sums,
                              const double* __restrict__ partial, int64_t cap, double* __restrict__ lambda) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_new) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t n = nd.scount[first + j];
  if (n < min_points) {
    lambda[first + j] = qnan;
    return;
  }
  double S[9];
  const int32_t b = base[j];
  if (b == -1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = sums[9 * j + k];
  } else {
    const int64_t nc = ((int64_t)nd.count[first + j] + NM_CHUNK - 1) / NM_CHUNK;
    if (b < 0 || (int64_t)b + nc > cap) {  // (unreachable: the work list is sized for every chunk)
      lambda[first + j] = qnan;
      return;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = partial[9 * (int64_t)b + k];
    for (int64_t c = 1; c < nc; ++c)
#pragma unroll
      for (int k = 0; k < 9; ++k) S[k] = S[k] + partial[9 * ((int64_t)b + c) + k];
  }
  // C = S_dd / (n - ddof) - n / (n - ddof) m m^T, m = S_d / n  (criteria.py: NotPlanar)
  const double dn = (double)n, dd = (double)(n - ddof);
  const double mx = S[0] / dn, my = S[1] / dn, mz = S[2] / dn;
  const double r = dn / dd;
  const double rx = r * mx, ry = r * my, rz = r * mz;
  double c6[6], w[3], v[9];
  c6[0] = fma(-rx, mx, S[3] / dd);
  c6[1] = fma(-rx, my, S[4] / dd);
  c6[2] = fma(-rx, mz, S[5] / dd);
  c6[3] = fma(-ry, my, S[6] / dd);
  c6[4] = fma(-ry, mz, S[7] / dd);
  c6[5] = fma(-rz, mz, S[8] / dd);
  sym3_eigen(c6, w, v);  // (values only: the vectors are dead code here)
  lambda[first + j] = w[0];
}

}  // namespace

int planar_level_stats(octl_forest* f, const PlanarRule& rule, NodeTable& nt, int64_t first_new, int64_t n_new,
                       const uint32_t* idx, const double* xyz, int xs, int64_t n_alive) {
  if (n_new <= 0) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  OCTL_TRY(devbuf_reserve(ctx, f->split_lambda, (size_t)std::max<int64_t>(nt.cap, first_new + n_new) * 8, 1));
  const int64_t cap = 2 * n_alive / NM_CHUNK + 2;
  // ctx->ls_buf: [sums 9 f64 per fresh node | chunk base i32 per fresh node | counter | work items int2 | chunk
  //               partials 9 f64], every part 256-byte aligned (never in flight together with leaf_stats: one stream)
  const size_t o_base = align256((size_t)n_new * 72);
  const size_t o_cnt = o_base + align256((size_t)n_new * 4);
  const size_t o_work = o_cnt + 256;
  const size_t o_part = o_work + align256((size_t)cap * 8);
  OCTL_TRY(devbuf_reserve(ctx, ctx->ls_buf, o_part + (size_t)cap * 72));
  char* b = static_cast<char*>(ctx->ls_buf.p);
  double* sums = reinterpret_cast<double*>(b);
  int32_t* base = reinterpret_cast<int32_t*>(b + o_base);
  uint32_t* counter = reinterpret_cast<uint32_t*>(b + o_cnt);
  int2* work = reinterpret_cast<int2*>(b + o_work);
  double* partial = reinterpret_cast<double*>(b + o_part);
  const NodePtrs nd = node_ptrs(nt);
  HIP_TRY(ctx, hipMemsetAsync(counter, 0, 16, st));
  {
    KTimer t(ctx, "node_moments");
    OCTL_LAUNCH(k_node_moments, dim3((unsigned)ceil_div(n_new, 16)), dim3(256), 0, st, nd, first_new, n_new,
                rule.min_points, idx, xyz, xs, counter, work, cap, base, sums);
    HIP_TRY(ctx, hipGetLastError());
    if (n_alive > NM_CHUNK) {  // (no node can exceed L positions otherwise)
      const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(ceil_div(cap, 4), (int64_t)octl_ctx_cus(ctx) * 8));
      OCTL_LAUNCH(k_node_chunks, dim3((unsigned)wgs), dim3(256), 0, st, (const uint32_t*)counter, (const int2*)work,
                  cap, nd, first_new, idx, xyz, xs, partial);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  {
    KTimer t(ctx, "node_lambda");
    OCTL_LAUNCH(k_node_lambda, dim3(grid_for(n_new)), dim3(256), 0, st, nd, first_new, n_new, rule.min_points,
                rule.ddof, (const int32_t*)base, (const double*)sums, (const double*)partial, cap,
                f->split_lambda.as<double>());
    HIP_TRY(ctx, hipGetLastError());
  }
  return OCTL_OK;
}

extern "C" int octl_forest_get_split_stats(octl_forest* f, int64_t cap, uint32_t* n_scheme, double* lambda_min,
                                           int64_t* n_nodes) {
  if (!f || !n_nodes) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  const int64_t total = f->nodes[f->cur].n;
  *n_nodes = total;
  const int64_t n = std::min<int64_t>(cap, total);
  if (n <= 0) return OCTL_OK;
  if (!f->split_stats_valid || f->split_stats_nodes != total) {
    // the scheme does not come from a planar build: no statistic was evaluated, no count kept
    if (n_scheme) std::memset(n_scheme, 0, (size_t)n * 4);
    if (lambda_min)
      for (int64_t i = 0; i < n; ++i) lambda_min[i] = __builtin_nan("");
    return OCTL_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n_scheme) HIP_TRY(ctx, hipMemcpyAsync(n_scheme, f->split_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  if (lambda_min)
    HIP_TRY(ctx, hipMemcpyAsync(lambda_min, f->split_lambda.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}
