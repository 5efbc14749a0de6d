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
// Launches: 2, in stream order; the host and the device form around them: reg_driver.h.  LDS: 960 bytes.
#include "common.h"
#include "forest.h"
#include "query_walk.h"
#include "reg_driver.h"
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
    double p[3];
    reg_transform(P.T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], p);
    const int32_t node = locate_one(t, p[0], p[1], p[2]);
    int32_t row;
    double nrm[3];
    const double r = plane_residual(pt, node, p[0], p[1], p[2], &row, nrm);
    if (PER_POINT) {
      node_out[i] = node;
      row_out[i] = row;
      res_out[i] = r;
    }
    a.located += node >= 0 ? 1 : 0;
    const double ar = fabs(r);
    if (!(row >= 0 && ar < INFINITY && !(P.max_distance >= 0.0 && ar > P.max_distance))) continue;  // (NaN: unused)
    a.used += 1;
    reg_plane_term(p[0], p[1], p[2], P.c, nrm, r, ar, P.huber_delta, a.s);  // (reg_plane_term.h fixes the order)
  }
  reg_block_reduce(a, lds, ldc);
  reg_write_row(a, rows);
}

struct RegCall {
  RegParams P;
  QueryTables t;
  PlaneTable pt;
};

// the checks every form starts with (state, then arguments: nothing has run when one of them fails)
int reg_begin(octl_forest* f, const void* xyz, int64_t n, const double* T, const double* origin, int32_t min_points,
              double max_variance, double max_distance, double huber_delta, const void* sys, const void* counts,
              bool columns_ok, RegCall* c) {
  OCTL_TRY(query_begin(f, "registration_system", &c->t));
  octl_ctx* ctx = f->ctx;
  OCTL_TRY(query_plane_table(f, "registration_system", min_points, max_variance, &c->pt));
  if (query_bad_count(n) || (n > 0 && !xyz) || !T || !origin || !sys || !counts || !columns_ok)
    return octl_set_error(ctx, OCTL_E_INVALID, "bad registration_system arguments");
  OCTL_TRY(reg_check_transform(ctx, "registration_system", T, origin));
  std::memcpy(c->P.T, T, sizeof c->P.T);
  std::memcpy(c->P.c, origin, sizeof c->P.c);
  c->P.max_distance = max_distance >= 0.0 ? max_distance : -1.0;
  c->P.huber_delta = huber_delta > 0.0 ? huber_delta : 0.0;
  return OCTL_OK;
}

// the two kernels of a call, as the forms of reg_driver.h enqueue them; columns: node, row, residual
auto reg_kernels(octl_ctx* ctx, const RegCall& c, int64_t n) {
  return [ctx, &c, n](const double* xyz_dev, void* const* col, const RegScratch& s, double* sys_dev,
                      int64_t* counts_dev) -> int {
    const int64_t n_rows = ceil_div(n, RS_CHUNK);
    {
      KTimer timer(ctx, "reg_partial");
      if (col[0])
        OCTL_LAUNCH(k_reg_partial<true>, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.t, c.pt,
                    (int32_t*)col[0], (int32_t*)col[1], (double*)col[2], s.rows);
      else
        OCTL_LAUNCH(k_reg_partial<false>, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.t, c.pt,
                    nullptr, nullptr, nullptr, s.rows);
      HIP_TRY(ctx, hipGetLastError());
    }
    return reg_fold_launch(ctx, s.rows, n_rows, sys_dev, counts_dev);
  };
}

}  // namespace

extern "C" {

int octl_forest_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                    const double origin[3], int32_t min_points, double max_variance,
                                    double max_distance, double huber_delta, double sys[28], int64_t counts[2],
                                    int32_t* node, int32_t* row, double* residual) {
  if (!f) return OCTL_E_INVALID;
  RegCall c;
  const RegColumn cols[] = {{node, 4}, {row, 4}, {residual, 8}};
  OCTL_TRY(reg_begin(f, xyz, n, T, origin, min_points, max_variance, max_distance, huber_delta, sys, counts,
                     reg_columns_ok(cols), &c));
  return reg_host_form(f, xyz, n, false, cols, sys, counts, reg_kernels(f->ctx, c, n));
}

int octl_forest_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n, const double T[12],
                                           const double origin[3], int32_t min_points, double max_variance,
                                           double max_distance, double huber_delta, double* sys_dev,
                                           int64_t* counts_dev, int32_t* node_dev, int32_t* row_dev,
                                           double* residual_dev) {
  if (!f) return OCTL_E_INVALID;
  RegCall c;
  const RegColumn cols[] = {{node_dev, 4}, {row_dev, 4}, {residual_dev, 8}};
  OCTL_TRY(reg_begin(f, xyz_dev, n, T, origin, min_points, max_variance, max_distance, huber_delta, sys_dev,
                     counts_dev, reg_columns_ok(cols), &c));
  return reg_device_form(f, xyz_dev, n, false, cols, sys_dev, counts_dev, reg_kernels(f->ctx, c, n));
}

}  // extern "C"
