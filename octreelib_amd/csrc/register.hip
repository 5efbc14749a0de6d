// Scan-to-map registration, the device's share: for ONE rigid transform T the point-to-plane normal equations of a
// scan against the pooled leaf planes (octl_forest_registration_system).  The 6x6 solve, the pose update and the
// iteration loop stay on the host (octreelib_amd/registration.py).  No reference counterpart: the reference has no
// registration.
//
// Per query q (octreelib_amd/registration.py: registration_system_np is the definition):
//   p = ((R_i0 q_x + R_i1 q_y) + R_i2 q_z) + t_i, every product and sum rounded (no fma: NumPy forms the same bits);
//   node = locate(p); row, r = the plane residual of octl_forest_point_to_plane (query_walk.h: the same code);
//   used iff row >= 0, r finite and |r| <= max_distance; an unused point is skipped, never multiplied by zero;
//   d = p - c, J = [d x n, n], w = 1 or Huber's min(1, delta / |r|);
//   H += w J J^T (21 upper-triangle entries), g += w J r (6), cost += rho(r): 28 sums, entered through fma.
//
// The summation tree is a function of n alone (no floating-point atomics, nothing depends on the CU count):
//   k_reg_partial  one workgroup of 256 per chunk of RS_CHUNK = 4096 consecutive queries; lane tid takes queries
//                  chunk * 4096 + j * 256 + tid, j = 0..15 in that order (at most 16 additions), then the wave's xor
//                  butterfly (32, 16, ..., 1: 6 additions), then the four waves in wave order through LDS (3), and the
//                  chunk's 28 sums + 2 counts go to row `chunk` of the scratch table;
//   k_reg_fold     one workgroup: thread k adds rows k, k + 256, ... in ascending order (ceil(rows / 256) additions),
//                  then the same butterfly (6) and wave-order fold (3).
// A term therefore passes through at most D = 16 + 6 + 3 + ceil(ceil(n / 4096) / 256) + 6 + 3 additions; forming it
// costs at most 8 more roundings (p - c, two per cross-product component, the weight's division, w J, the products).
//
// Launches: 2, in stream order.  The host form adds one upload, the download of the 28 + 2 numbers (and of the
// per-point answers when asked for) and ONE host wait; the device form does not wait.  LDS: 960 bytes.
#include <cmath>

#include "common.h"
#include "forest.h"
#include "query_walk.h"
#include "reg_fold.h"
#include "reg_plane_term.h"

namespace {

struct RegParams {
  double T[12];         // row-major 3 x 4: R | t
  double c[3];          // origin of the rotational part
  double max_distance;  // < 0: no gate
  double huber_delta;   // <= 0: no weights
};

template <bool PER_POINT>
__global__ __launch_bounds__(256) void k_reg_partial(const double* __restrict__ xyz, int64_t n, RegParams P,
                                                     QueryTables t, PlaneTable pt, int32_t* __restrict__ node_out,
                                                     int32_t* __restrict__ row_out, double* __restrict__ res_out,
                                                     double* __restrict__ rows) {
  __shared__ double lds[4][RS_SUMS];
  __shared__ long long ldc[4][2];
  RegAcc a;
  reg_zero(a);
  const int64_t base = (int64_t)blockIdx.x * RS_CHUNK + threadIdx.x;
#pragma unroll 1
  for (int j = 0; j < RS_CHUNK / 256; ++j) {
    const int64_t i = base + (int64_t)j * 256;
    if (i >= n) break;
    const double qx = xyz[3 * i + 0], qy = xyz[3 * i + 1], qz = xyz[3 * i + 2];
    // (separate products and sums: the library is built with -ffp-contract=off, and the host forms the same bits)
    const double px = ((P.T[0] * qx + P.T[1] * qy) + P.T[2] * qz) + P.T[3];
    const double py = ((P.T[4] * qx + P.T[5] * qy) + P.T[6] * qz) + P.T[7];
    const double pz = ((P.T[8] * qx + P.T[9] * qy) + P.T[10] * qz) + P.T[11];
    const int32_t node = locate_one(t, px, py, pz);
    int32_t row;
    double nrm[3];
    const double r = plane_residual(pt, node, px, py, pz, &row, nrm);
    if (PER_POINT) {
      node_out[i] = node;
      row_out[i] = row;
      res_out[i] = r;
    }
    a.located += node >= 0 ? 1 : 0;
    const double ar = fabs(r);
    if (!(row >= 0 && ar < INFINITY && !(P.max_distance >= 0.0 && ar > P.max_distance))) continue;  // (NaN: unused)
    a.used += 1;
    reg_plane_term(px, py, pz, P.c, nrm, r, ar, P.huber_delta, a.s);  // (reg_plane_term.h fixes the operation order)
  }
  reg_block_reduce(a, lds, ldc);
  double* out = rows + (int64_t)blockIdx.x * RS_ROW;
  if (threadIdx.x < RS_SUMS) out[threadIdx.x] = a.s[0];
  if (threadIdx.x == 0) {
    reinterpret_cast<long long*>(out)[RS_SUMS] = a.used;
    reinterpret_cast<long long*>(out)[RS_SUMS + 1] = a.located;
  }
}

struct RegCall {
  RegParams P;
  QueryTables t;
  PlaneTable pt;
};

// the checks every form starts with (state, then arguments: nothing has run when one of them fails)
int reg_begin(octl_forest* f, const void* xyz, int64_t n, const double* T, const double* origin, int32_t min_points,
              double max_variance, double max_distance, double huber_delta, const void* sys, const void* counts,
              const void* node, const void* row, const void* residual, RegCall* c) {
  OCTL_TRY(query_begin(f, "registration_system", &c->t));
  octl_ctx* ctx = f->ctx;
  OCTL_TRY(query_plane_table(f, "registration_system", min_points, max_variance, &c->pt));
  const int per_point = (node ? 1 : 0) + (row ? 1 : 0) + (residual ? 1 : 0);
  if (query_bad_count(n) || (n > 0 && !xyz) || !T || !origin || !sys || !counts || (per_point != 0 && per_point != 3))
    return octl_set_error(ctx, OCTL_E_INVALID, "bad registration_system arguments");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(T[k]))
      return octl_set_error(ctx, OCTL_E_INVALID, "registration_system: the transform is not finite");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k]))
      return octl_set_error(ctx, OCTL_E_INVALID, "registration_system: the origin is not finite");
  std::memcpy(c->P.T, T, sizeof c->P.T);
  std::memcpy(c->P.c, origin, sizeof c->P.c);
  c->P.max_distance = max_distance >= 0.0 ? max_distance : -1.0;
  c->P.huber_delta = huber_delta > 0.0 ? huber_delta : 0.0;
  return OCTL_OK;
}

// the two kernels; rows_dev holds ceil(n / RS_CHUNK) rows
int reg_launch(octl_ctx* ctx, const RegCall& c, const double* xyz_dev, int64_t n, int32_t* node, int32_t* row,
               double* residual, double* rows_dev, double* sys_dev, int64_t* counts_dev) {
  const int64_t n_rows = ceil_div(n, RS_CHUNK);
  {
    KTimer timer(ctx, "reg_partial");
    if (node)
      OCTL_LAUNCH(k_reg_partial<true>, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.t, c.pt,
                  node, row, residual, rows_dev);
    else
      OCTL_LAUNCH(k_reg_partial<false>, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.t, c.pt,
                  nullptr, nullptr, nullptr, rows_dev);
    HIP_TRY(ctx, hipGetLastError());
  }
  KTimer timer(ctx, "reg_fold");
  OCTL_LAUNCH(k_reg_fold, dim3(1), dim3(256), 0, ctx->stream, rows_dev, n_rows, sys_dev, counts_dev);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

// scratch of one call in f->rg_rows: [0, 256) the result (28 sums, 2 counts), then the rows
int reg_scratch(octl_forest* f, int64_t n, double** result, double** rows) {
  OCTL_TRY(devbuf_reserve(f->ctx, f->rg_rows, 256 + (size_t)ceil_div(n, RS_CHUNK) * RS_ROW * 8));
  *result = f->rg_rows.as<double>();
  *rows = f->rg_rows.as<double>() + 32;
  return OCTL_OK;
}

}  // namespace

extern "C" {

int octl_forest_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                    const double origin[3], int32_t min_points, double max_variance,
                                    double max_distance, double huber_delta, double sys[28], int64_t counts[2],
                                    int32_t* node, int32_t* row, double* residual) {
  if (!f) return OCTL_E_INVALID;
  RegCall c;
  OCTL_TRY(reg_begin(f, xyz, n, T, origin, min_points, max_variance, max_distance, huber_delta, sys, counts, node, row,
                     residual, &c));
  if (n == 0) {
    for (int k = 0; k < RS_SUMS; ++k) sys[k] = 0.0;
    counts[0] = counts[1] = 0;
    return OCTL_OK;
  }
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const size_t o_node = align256((size_t)n * 24), o_row = o_node + align256((size_t)n * 4);
  const size_t o_res = o_row + align256((size_t)n * 4);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, node ? o_res + (size_t)n * 8 : o_node));
  double *result_d = nullptr, *rows_d = nullptr;
  OCTL_TRY(reg_scratch(f, n, &result_d, &rows_d));
  char* base = static_cast<char*>(f->q_stage.p);
  int32_t* node_d = node ? reinterpret_cast<int32_t*>(base + o_node) : nullptr;
  int32_t* row_d = node ? reinterpret_cast<int32_t*>(base + o_row) : nullptr;
  double* res_d = node ? reinterpret_cast<double*>(base + o_res) : nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(base, xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OCTL_TRY(reg_launch(ctx, c, reinterpret_cast<const double*>(base), n, node_d, row_d, res_d, rows_d, result_d,
                      reinterpret_cast<int64_t*>(result_d + RS_SUMS)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->small_host, result_d, (RS_SUMS + 2) * 8, hipMemcpyDeviceToHost, st));
  if (node) {
    HIP_TRY(ctx, hipMemcpyAsync(node, node_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(row, row_d, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(residual, res_d, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memcpy(sys, ctx->small_host, RS_SUMS * 8);
  std::memcpy(counts, static_cast<const char*>(ctx->small_host) + RS_SUMS * 8, 16);
  return OCTL_OK;
}

int octl_forest_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n, const double T[12],
                                           const double origin[3], int32_t min_points, double max_variance,
                                           double max_distance, double huber_delta, double* sys_dev,
                                           int64_t* counts_dev, int32_t* node_dev, int32_t* row_dev,
                                           double* residual_dev) {
  if (!f) return OCTL_E_INVALID;
  RegCall c;
  OCTL_TRY(reg_begin(f, xyz_dev, n, T, origin, min_points, max_variance, max_distance, huber_delta, sys_dev,
                     counts_dev, node_dev, row_dev, residual_dev, &c));
  octl_ctx* ctx = f->ctx;
  if (n == 0) {  // (nothing to reduce: the zeros are two fills in stream order)
    HIP_TRY(ctx, hipMemsetAsync(sys_dev, 0, RS_SUMS * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, 16, ctx->stream));
    return OCTL_OK;
  }
  double *result_d = nullptr, *rows_d = nullptr;
  OCTL_TRY(reg_scratch(f, n, &result_d, &rows_d));
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  return reg_launch(ctx, c, xyz_dev, n, node_dev, row_dev, residual_dev, rows_d, sys_dev, counts_dev);
}

}  // extern "C"
