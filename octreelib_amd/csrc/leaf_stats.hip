// Per-(leaf, pose) point statistics on the device: count, mean, population covariance and its eigen-decomposition
// for a list of blocks of the forest's block table (octl_forest_leaf_stats).  The points are already leaf-ordered
// in xyz_ord and every block is one run [blk_start, blk_start + blk_size) of it, so the whole job is a segmented
// reduction plus one 3x3 eigensolve per block.
//
// The moments of a block with anchor p0 = its first point in storage order are
//   S = sum over the block's chunks c = 0, 1, ... (in that order) of P_c,
//   P_c = the 64-lane reduction of chunk c = points [c L, min((c+1) L, n)) of the block: lane l accumulates
//         d = p - p0 over the chunk's points l, l+64, ... (sums of d and of d d^T, f64, fma), then a butterfly
//         (xor 32, 16, ..., 1) that leaves the totals in every lane.
// mean = p0 + S_d / n, cov = S_dd / n - (S_d / n)(S_d / n)^T.  The shift is what makes the one-pass form safe:
// cancellation is relative to the block's extent, not to the magnitude of its coordinates.  S depends on the
// block's points and nothing else - not on where the block sits in the store, not on the other requested blocks -
// so a block's results are the same bits however it is requested.
//
// Launches (stream order, one host wait for the download):
//   [fill]          claim words of the block table + chunk counter (only when a block can exceed L points)
//   k_leaf_moments  one wave per requested block: a block of at most L points is reduced and finished here; a
//                   larger one is claimed by the first request that meets it, which books ceil(n / L) work items
//   k_leaf_chunks   [only when a block can exceed L points] one wave per work item (grid-stride): P_c of one chunk
//   k_leaf_eigen    one lane per requested block: folds the chunk partials of a large block in chunk order and
//                   finishes it, then the cyclic Jacobi of sym3_eigen.h
// A forest whose blocks are known to hold at most L points (a count-driven build with K <= L) skips the fill and
// k_leaf_chunks; should a larger block appear anyway, k_leaf_moments folds its chunks itself, in the same order and
// with the same arithmetic - the same bits, only slower.
#include <algorithm>

#include "common.h"
#include "forest.h"
#include "sym3_eigen.h"

namespace {

constexpr int LS_CHUNK = 64 * 64;  // L: points per chunk of a large block

struct Sums {
  double s[9];  // sum dx, dy, dz; sum dx dx, dx dy, dx dz, dy dy, dy dz, dz dz
};

// P_c: the moments of points [first, first + cnt) relative to p0, reduced over the wave; every lane returns them
__device__ __forceinline__ Sums chunk_sums(const double* __restrict__ xyz, int64_t first, int cnt, double p0x,
                                           double p0y, double p0z, int lane) {
  Sums a;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.s[k] = 0.0;
  for (int j = lane; j < cnt; j += 64) {
    const double* p = xyz + 3 * (first + j);
    const double dx = p[0] - p0x, dy = p[1] - p0y, dz = p[2] - p0z;
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
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int k = 0; k < 9; ++k) a.s[k] += __shfl_xor(a.s[k], m);
  return a;
}

__device__ __forceinline__ void fold(Sums& acc, const Sums& p) {
#pragma unroll
  for (int k = 0; k < 9; ++k) acc.s[k] = acc.s[k] + p.s[k];
}

__device__ __forceinline__ void finish(const Sums& S, int64_t n, double p0x, double p0y, double p0z, double* mean,
                                       double* cov) {
  const double dn = (double)n;
  const double mx = S.s[0] / dn, my = S.s[1] / dn, mz = S.s[2] / dn;
  mean[0] = p0x + mx;
  mean[1] = p0y + my;
  mean[2] = p0z + mz;
  cov[0] = fma(-mx, mx, S.s[3] / dn);
  cov[1] = fma(-mx, my, S.s[4] / dn);
  cov[2] = fma(-mx, mz, S.s[5] / dn);
  cov[3] = fma(-my, my, S.s[6] / dn);
  cov[4] = fma(-my, mz, S.s[7] / dn);
  cov[5] = fma(-mz, mz, S.s[8] / dn);
}

__global__ __launch_bounds__(256) void k_leaf_moments(const int32_t* __restrict__ ids, int64_t nb,
                                                      const uint32_t* __restrict__ blk_start,
                                                      const int32_t* __restrict__ blk_size,
                                                      const double* __restrict__ xyz, int chunked,
                                                      int32_t* __restrict__ claim, uint32_t* __restrict__ counter,
                                                      int2* __restrict__ work, int64_t cap,
                                                      int64_t* __restrict__ count, double* __restrict__ mean,
                                                      double* __restrict__ cov) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nb) return;
  const int lane = threadIdx.x & 63;
  const int32_t b = ids[i];
  const int64_t s = blk_start[b];
  const int32_t n = blk_size[b];
  if (lane == 0) count[i] = n;
  if (n <= 0) {  // (the table holds non-empty blocks only)
    if (lane < 3) mean[3 * i + lane] = 0.0;
    if (lane < 6) cov[6 * i + lane] = 0.0;
    return;
  }
  if (chunked && n > LS_CHUNK) {
    // the first request of this block books its chunks; k_leaf_chunks reduces them, k_leaf_eigen folds them
    const int32_t nc = (n + LS_CHUNK - 1) / LS_CHUNK;
    int32_t off = -1;
    if (lane == 0 && atomicCAS(&claim[b], 0, -2) == 0) {
      const uint32_t o = atomicAdd(counter, (uint32_t)nc);
      const bool fits = (int64_t)o + nc <= cap;  // (always: the chunks of distinct blocks number < 2 n_ord / L)
      claim[b] = fits ? (int32_t)o + 1 : -1;
      off = fits ? (int32_t)o : -1;
    }
    off = __shfl(off, 0);
    if (off >= 0)
      for (int c = lane; c < nc; c += 64) work[off + c] = make_int2(b, c);
    return;
  }
  const double p0x = xyz[3 * s], p0y = xyz[3 * s + 1], p0z = xyz[3 * s + 2];
  Sums S = chunk_sums(xyz, s, min(n, LS_CHUNK), p0x, p0y, p0z, lane);
  for (int32_t c0 = LS_CHUNK; c0 < n; c0 += LS_CHUNK)  // (a large block on a forest without the chunk stage)
    fold(S, chunk_sums(xyz, s + c0, min(n - c0, LS_CHUNK), p0x, p0y, p0z, lane));
  if (lane == 0) finish(S, n, p0x, p0y, p0z, mean + 3 * i, cov + 6 * i);
}

__global__ __launch_bounds__(256) void k_leaf_chunks(const uint32_t* __restrict__ counter,
                                                     const int2* __restrict__ work, int64_t cap,
                                                     const uint32_t* __restrict__ blk_start,
                                                     const int32_t* __restrict__ blk_size,
                                                     const double* __restrict__ xyz, double* __restrict__ partial) {
  const int64_t total = min((int64_t)*counter, cap);
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < total; t += waves) {
    const int2 w = work[t];
    const int64_t s = blk_start[w.x];
    const int32_t n = blk_size[w.x];
    const int32_t c0 = w.y * LS_CHUNK;
    const Sums P = chunk_sums(xyz, s + c0, min(n - c0, LS_CHUNK), xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2], lane);
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < 9; ++k) partial[9 * t + k] = P.s[k];
  }
}

__global__ __launch_bounds__(256) void k_leaf_eigen(const int32_t* __restrict__ ids, int64_t nb,
                                                    const uint32_t* __restrict__ blk_start,
                                                    const int32_t* __restrict__ blk_size,
                                                    const double* __restrict__ xyz, int chunked,
                                                    const int32_t* __restrict__ claim, int64_t cap,
                                                    const double* __restrict__ partial, double* __restrict__ mean,
                                                    double* __restrict__ cov, double* __restrict__ eigval,
                                                    double* __restrict__ eigvec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  double c6[6];
  const int32_t b = ids[i];
  const int32_t n = blk_size[b];
  if (chunked && n > LS_CHUNK) {
    const int32_t nc = (n + LS_CHUNK - 1) / LS_CHUNK;
    const int64_t base = (int64_t)claim[b] - 1;
    const int64_t s = blk_start[b];
    double m3[3];
    if (base >= 0 && base + nc <= cap) {
      Sums S;
#pragma unroll
      for (int k = 0; k < 9; ++k) S.s[k] = partial[9 * base + k];
      for (int32_t c = 1; c < nc; ++c) {
        Sums P;
#pragma unroll
        for (int k = 0; k < 9; ++k) P.s[k] = partial[9 * (base + c) + k];
        fold(S, P);
      }
      finish(S, n, xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2], m3, c6);
    } else {  // (unreachable: the work list is sized for every chunk)
      const double q = __longlong_as_double(0x7ff8000000000000ll);
      m3[0] = m3[1] = m3[2] = q;
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = q;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[3 * i + k] = m3[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) cov[6 * i + k] = c6[k];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov[6 * i + k];
  }
  if (!eigval) return;
  double w[3], v[9];
  sym3_eigen(c6, w, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) eigval[3 * i + k] = w[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) eigvec[9 * i + k] = v[k];
}

__global__ __launch_bounds__(256) void k_sym3_eigen(const double* __restrict__ c6, int64_t n,
                                                    double* __restrict__ eigval, double* __restrict__ eigvec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double c[6], w[3], v[9];
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = c6[6 * i + k];
  sym3_eigen(c, w, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) eigval[3 * i + k] = w[k];
#pragma unroll
  for (int k = 0; k < 9; ++k) eigvec[9 * i + k] = v[k];
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" int octl_forest_leaf_stats(octl_forest* f, const int32_t* block_ids, int64_t nb, int64_t* count,
                                      double* mean, double* cov, double* eigval, double* eigvec) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "leaf_stats before build");
  if (nb < 0 || (nb > 0 && !block_ids)) return octl_set_error(ctx, OCTL_E_INVALID, "bad leaf_stats arguments");
  if (nb >= ((int64_t)1 << 31)) return octl_set_error(ctx, OCTL_E_INVALID, "too many blocks in one leaf_stats call");
  for (int64_t i = 0; i < nb; ++i)
    if (block_ids[i] < 0 || block_ids[i] >= f->n_blocks)
      return octl_set_error(ctx, OCTL_E_INVALID, "block index %lld out of range [0, %lld)", (long long)block_ids[i],
                            (long long)f->n_blocks);
  if (nb == 0) return OCTL_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool eigen = eigval || eigvec;
  const bool chunked = f->max_block_hint > LS_CHUNK;
  // at most ceil(n / L) < 2 n / L chunks per block of n > L points, and the blocks are disjoint runs of xyz_ord
  const int64_t cap = chunked ? 2 * f->n_ord / LS_CHUNK + 2 : 0;
  // ctx->ls_buf: [ids i32 | count i64 | mean 3 f64 | cov 6 f64 | eigval 3 f64 | eigvec 9 f64 | counter + claim i32
  //               per table block | work items int2 | chunk partials 9 f64], every part 256-byte aligned
  const size_t o_cnt = align256((size_t)nb * 4);
  const size_t o_mean = o_cnt + align256((size_t)nb * 8);
  const size_t o_cov = o_mean + align256((size_t)nb * 24);
  const size_t o_w = o_cov + align256((size_t)nb * 48);
  const size_t o_v = o_w + (eigen ? align256((size_t)nb * 24) : 0);
  const size_t o_claim = o_v + (eigen ? align256((size_t)nb * 72) : 0);
  const size_t claim_bytes = chunked ? 16 + (size_t)f->n_blocks * 4 : 0;
  const size_t o_work = o_claim + align256(claim_bytes);
  const size_t o_part = o_work + align256((size_t)cap * 8);
  const size_t total = o_part + (size_t)cap * 72;
  OCTL_TRY(devbuf_reserve(ctx, ctx->ls_buf, total));
  char* base = static_cast<char*>(ctx->ls_buf.p);
  int32_t* ids_d = reinterpret_cast<int32_t*>(base);
  int64_t* cnt_d = reinterpret_cast<int64_t*>(base + o_cnt);
  double* mean_d = reinterpret_cast<double*>(base + o_mean);
  double* cov_d = reinterpret_cast<double*>(base + o_cov);
  double* w_d = eigen ? reinterpret_cast<double*>(base + o_w) : nullptr;
  double* v_d = eigen ? reinterpret_cast<double*>(base + o_v) : nullptr;
  uint32_t* counter_d = reinterpret_cast<uint32_t*>(base + o_claim);
  int32_t* claim_d = reinterpret_cast<int32_t*>(base + o_claim + 16);
  int2* work_d = reinterpret_cast<int2*>(base + o_work);
  double* part_d = reinterpret_cast<double*>(base + o_part);
  const uint32_t* bstart = f->blk_start.as<uint32_t>();
  const int32_t* bsize = f->blk_size.as<int32_t>();
  const double* xyz = f->xyz_ord.as<double>();

  HIP_TRY(ctx, hipMemcpyAsync(ids_d, block_ids, (size_t)nb * 4, hipMemcpyHostToDevice, st));
  if (chunked) HIP_TRY(ctx, hipMemsetAsync(counter_d, 0, claim_bytes, st));
  {
    KTimer t(ctx, "leaf_moments");
    OCTL_LAUNCH(k_leaf_moments, dim3((unsigned)ceil_div(nb, 4)), dim3(256), 0, st, (const int32_t*)ids_d, nb, bstart,
                bsize, xyz, (int)chunked, claim_d, counter_d, work_d, cap, cnt_d, mean_d, cov_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (chunked) {
    KTimer t(ctx, "leaf_chunks");
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(ceil_div(cap, 4), (int64_t)octl_ctx_cus(ctx) * 8));
    OCTL_LAUNCH(k_leaf_chunks, dim3((unsigned)wgs), dim3(256), 0, st, (const uint32_t*)counter_d,
                (const int2*)work_d, cap, bstart, bsize, xyz, part_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (chunked || eigen) {
    KTimer t(ctx, "leaf_eigen");
    OCTL_LAUNCH(k_leaf_eigen, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, st, (const int32_t*)ids_d, nb, bstart,
                bsize, xyz, (int)chunked, (const int32_t*)claim_d, cap, (const double*)part_d, mean_d, cov_d, w_d,
                v_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (count) HIP_TRY(ctx, hipMemcpyAsync(count, cnt_d, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
  if (mean) HIP_TRY(ctx, hipMemcpyAsync(mean, mean_d, (size_t)nb * 24, hipMemcpyDeviceToHost, st));
  if (cov) HIP_TRY(ctx, hipMemcpyAsync(cov, cov_d, (size_t)nb * 48, hipMemcpyDeviceToHost, st));
  if (eigval) HIP_TRY(ctx, hipMemcpyAsync(eigval, w_d, (size_t)nb * 24, hipMemcpyDeviceToHost, st));
  if (eigvec) HIP_TRY(ctx, hipMemcpyAsync(eigvec, v_d, (size_t)nb * 72, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

extern "C" int octl_debug_sym3_eigen(octl_ctx* ctx, const double* cov6, int64_t n, double* eigval, double* eigvec) {
  if (!ctx) return OCTL_E_INVALID;
  if (n < 0 || (n > 0 && (!cov6 || !eigval || !eigvec)))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad sym3_eigen arguments");
  if (n == 0) return OCTL_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t o_w = align256((size_t)n * 48), o_v = o_w + align256((size_t)n * 24);
  OCTL_TRY(devbuf_reserve(ctx, ctx->ls_buf, o_v + (size_t)n * 72));
  char* base = static_cast<char*>(ctx->ls_buf.p);
  HIP_TRY(ctx, hipMemcpyAsync(base, cov6, (size_t)n * 48, hipMemcpyHostToDevice, st));
  OCTL_LAUNCH(k_sym3_eigen, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, (const double*)base, n,
              reinterpret_cast<double*>(base + o_w), reinterpret_cast<double*>(base + o_v));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(eigval, base + o_w, (size_t)n * 24, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(eigvec, base + o_v, (size_t)n * 72, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}
