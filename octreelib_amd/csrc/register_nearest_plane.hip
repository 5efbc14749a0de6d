// Nearest-point-to-plane scan-to-map registration, the device's share: for ONE rigid transform T the point-to-plane
// normal equations of a scan, every transformed query scored against the pooled plane of the leaf its NEAREST STORED
// POINT lies in (octl_forest_nearest_plane_registration_system).  The correspondence is that of
// octl_forest_point_registration_system (4.19: the basin is max_distance, not a leaf), the residual that of
// octl_forest_registration_system (4.9: the scan slides along a plane instead of creeping to the map's samples).  The
// 6x6 solve, the pose update and the loop stay on the host (octreelib_amd/registration.py:
// nearest_plane_registration_system_np is the definition, align_np the loop).  No reference counterpart: the reference
// has no registration.
//
// Per query q:
//   p = ((R_i0 q_x + R_i1 q_y) + R_i2 q_z) + t_i, every product and sum rounded (the bits of transform_np);
//   the nearest stored point m of the selection within max_distance: the search of octl_forest_nearest with k = 1
//   (nearest_walk.h - the same cubes, the same d2 bits, the same total order (d2, slot, index));
//   node = locate(m), the scheme leaf the matched point lies in (-1: no match) - NOT locate(p);
//   row, r = the residual of p against the pooled plane of `node` (query_walk.h: plane_residual, the code of
//   octl_forest_point_to_plane); used iff row >= 0 and r finite; located iff node >= 0;
//   the point's term of the 28 sums: reg_plane_term.h, the code of k_reg_partial.
//
// Three launches in stream order:
//   k_regn_match   one query per lane, grid-stride, launched as k_reg_match is: the walk, then - for a matched query -
//                  one descent and one 64-byte plane gather; writes one 32-byte record {n, r} per query and, in its
//                  second instance, slot / index / distance2 / node / row / residual.  r of a record: the residual, NaN
//                  (correspondence, no accepted plane) or the NaN of REGN_NO_MATCH's bits (no correspondence);
//   k_regn_partial the summation tree of k_reg_partial unchanged (register.hip): chunks of 4096, lane tid takes
//                  4096 k + 256 j + tid for j = 0..15 in that order, reg_block_reduce, row k.  No walk: 56 bytes per
//                  query streamed;
//   k_reg_fold     as it is (reg_fold.h).
// The tree is a function of n alone: no floating-point atomics, nothing sized by the CU count (the grid of k_regn_match
// is, and it adds nothing).  The host and the device form around the launches: reg_driver.h.  LDS: 960 bytes
// (k_regn_partial, k_reg_fold), none in k_regn_match.
#include "common.h"
#include "forest.h"
#include "nearest_walk.h"
#include "reg_best.h"
#include "reg_driver.h"
#include "reg_fold.h"
#include "reg_plane_term.h"

namespace {

struct RegNParams {
  double T[12];  // row-major 3 x 4: R | t
  double c[3];   // origin of the rotational part
  double delta;  // <= 0: no weights
};

// r of the record of a query without a correspondence: a quiet NaN no operation produces (plane_residual answers the
// NaN of payload 0 for "no accepted plane"); told apart by its bits
constexpr long long REGN_NO_MATCH = 0x7ff8000000000001ll;

template <bool PER_POINT>
__global__ __launch_bounds__(256) void k_regn_match(const double* __restrict__ xyz, int64_t n, RegNParams P, double r,
                                                    double r2, NNTables T, PlaneTable pt, double4* __restrict__ rec_out,
                                                    int32_t* __restrict__ slot_out, int64_t* __restrict__ index_out,
                                                    double* __restrict__ d2_out, int32_t* __restrict__ node_out,
                                                    int32_t* __restrict__ row_out, double* __restrict__ res_out) {
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double p[3];
    reg_transform(P.T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], p);
    RegBest best = {INF, ~0ull, 0u};
    nearest_walk(T, p[0], p[1], p[2], r, r2, best);
    const bool has = best.bid != ~0ull;
    int32_t node = -1, row = -1;
    double nrm[3] = {0.0, 0.0, 0.0};
    double res = __longlong_as_double(0x7ff8000000000000ll);
    if (has) {
      // (the leaf of the matched point, by the descent every query takes: the walk is not asked for it)
      const double* __restrict__ m = T.xyz_ord + 3 * (int64_t)best.pos;
      node = locate_one(T.t, m[0], m[1], m[2]);
      res = plane_residual(pt, node, p[0], p[1], p[2], &row, nrm);
    }
    rec_out[i] = make_double4(nrm[0], nrm[1], nrm[2], node >= 0 ? res : __longlong_as_double(REGN_NO_MATCH));
    if (PER_POINT) {
      slot_out[i] = has ? (int32_t)(best.bid >> 32) : -1;
      index_out[i] = has ? (int64_t)(best.bid & 0xffffffffull) : -1;
      d2_out[i] = best.bd;
      node_out[i] = node;
      row_out[i] = row;
      res_out[i] = res;
    }
  }
}

__global__ __launch_bounds__(256) void k_regn_partial(const double* __restrict__ xyz, int64_t n, RegNParams P,
                                                      const double4* __restrict__ rec, double* __restrict__ rows) {
  __shared__ double lds[4][RS_SUMS];
  __shared__ long long ldc[4][2];
  RegAcc a;
  reg_zero(a);
  const int64_t base = (int64_t)blockIdx.x * RS_CHUNK + threadIdx.x;
#pragma unroll 1
  for (int j = 0; j < RS_CHUNK / 256; ++j) {
    const int64_t i = base + (int64_t)j * 256;
    if (i >= n) break;
    const double4 m = rec[i];
    a.located += __double_as_longlong(m.w) != REGN_NO_MATCH ? 1 : 0;
    const double ar = fabs(m.w);
    if (!(ar < INFINITY)) continue;  // (NaN: no correspondence or no accepted plane - skipped, never multiplied by zero)
    a.used += 1;
    double p[3];
    reg_transform(P.T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], p);
    const double nrm[3] = {m.x, m.y, m.z};
    reg_plane_term(p[0], p[1], p[2], P.c, nrm, m.w, ar, P.delta, a.s);
  }
  reg_block_reduce(a, lds, ldc);
  reg_write_row(a, rows);
}

struct RegNCall {
  RegNParams P;
  NNTables T;
  PlaneTable pt;
  double r;
};

const char* const WHAT = "nearest_plane_registration_system";

// the same poses, whichever way "all of them" is written (empty: every pose)
bool same_selection(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int n_poses) {
  for (int s = 0; s < n_poses; ++s)
    if ((a.empty() || a[(size_t)s]) != (b.empty() || b[(size_t)s])) return false;
  return true;
}

// the checks every form starts with (nothing has run when one of them fails): the search's in its order, then the
// system's, then that planes and points come from the same poses; the block index is made last
int regn_begin(octl_forest* f, const void* xyz, int64_t n, const double* T, const double* origin, int32_t min_points,
               double max_variance, double max_distance, double huber_delta, const uint8_t* slot_sel, int32_t n_sel,
               const void* sys, const void* counts, bool columns_ok, RegNCall* c) {
  const bool pointers_ok = (n <= 0 || xyz) && T && origin && sys && counts && columns_ok;
  octl_ctx* ctx = f->ctx;
  // (nearest_begin ends by making the block index; with n = 0 it stops after its refusals, so the count is tested here)
  OCTL_TRY(nearest_begin(f, WHAT, 0, 1, max_distance, slot_sel, n_sel, pointers_ok && !query_bad_count(n), &c->T));
  OCTL_TRY(reg_check_transform(ctx, WHAT, T, origin));
  OCTL_TRY(query_plane_table(f, WHAT, min_points, max_variance, &c->pt));
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  if (!same_selection(f->pl_sel, sel, (int)f->pose_off.size() - 1))
    return octl_set_error(ctx, OCTL_E_STATE,
                          "%s: the pooled leaf planes were made for another pose selection than the one searched - "
                          "call octl_forest_pooled_leaf_stats with this selection first",
                          WHAT);
  OCTL_TRY(nearest_begin(f, WHAT, n, 1, max_distance, slot_sel, n_sel, true, &c->T));
  std::memcpy(c->P.T, T, sizeof c->P.T);
  std::memcpy(c->P.c, origin, sizeof c->P.c);
  c->P.delta = huber_delta > 0.0 ? huber_delta : 0.0;
  c->r = max_distance;
  return OCTL_OK;
}

// the three kernels of a call, as the forms of reg_driver.h enqueue them; columns: slot, index, distance2, node, row,
// residual
auto regn_kernels(octl_ctx* ctx, const RegNCall& c, int64_t n) {
  return [ctx, &c, n](const double* xyz_dev, void* const* col, const RegScratch& s, double* sys_dev,
                      int64_t* counts_dev) -> int {
    const int64_t n_rows = ceil_div(n, RS_CHUNK);
    const double r2 = c.r * c.r;
    {
      KTimer timer(ctx, "regn_match");
      const unsigned wgs = grid_stride_for(ctx, n);
      if (col[0])
        OCTL_LAUNCH(k_regn_match<true>, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.r, r2, c.T, c.pt,
                    s.rec, (int32_t*)col[0], (int64_t*)col[1], (double*)col[2], (int32_t*)col[3], (int32_t*)col[4],
                    (double*)col[5]);
      else
        OCTL_LAUNCH(k_regn_match<false>, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.r, r2, c.T, c.pt,
                    s.rec, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
      HIP_TRY(ctx, hipGetLastError());
    }
    {
      KTimer timer(ctx, "regn_partial");
      OCTL_LAUNCH(k_regn_partial, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, xyz_dev, n, c.P,
                  (const double4*)s.rec, s.rows);
      HIP_TRY(ctx, hipGetLastError());
    }
    return reg_fold_launch(ctx, s.rows, n_rows, sys_dev, counts_dev);
  };
}

}  // namespace

extern "C" {

int octl_forest_nearest_plane_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                                  const double origin[3], double max_distance, double huber_delta,
                                                  const uint8_t* slot_sel, int32_t n_sel, int32_t min_points,
                                                  double max_variance, double sys[28], int64_t counts[2],
                                                  int32_t* slot, int64_t* index, double* distance2, int32_t* node,
                                                  int32_t* row, double* residual) {
  if (!f) return OCTL_E_INVALID;
  RegNCall c;
  const RegColumn cols[] = {{slot, 4}, {index, 8}, {distance2, 8}, {node, 4}, {row, 4}, {residual, 8}};
  OCTL_TRY(regn_begin(f, xyz, n, T, origin, min_points, max_variance, max_distance, huber_delta, slot_sel, n_sel, sys,
                      counts, reg_columns_ok(cols), &c));
  return reg_host_form(f, xyz, n, true, cols, sys, counts, regn_kernels(f->ctx, c, n));
}

int octl_forest_nearest_plane_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n,
                                                         const double T[12], const double origin[3],
                                                         double max_distance, double huber_delta,
                                                         const uint8_t* slot_sel, int32_t n_sel, int32_t min_points,
                                                         double max_variance, double* sys_dev, int64_t* counts_dev,
                                                         int32_t* slot_dev, int64_t* index_dev, double* distance2_dev,
                                                         int32_t* node_dev, int32_t* row_dev, double* residual_dev) {
  if (!f) return OCTL_E_INVALID;
  RegNCall c;
  const RegColumn cols[] = {{slot_dev, 4},     {index_dev, 8}, {distance2_dev, 8},
                            {node_dev, 4},     {row_dev, 4},   {residual_dev, 8}};
  OCTL_TRY(regn_begin(f, xyz_dev, n, T, origin, min_points, max_variance, max_distance, huber_delta, slot_sel, n_sel,
                      sys_dev, counts_dev, reg_columns_ok(cols), &c));
  return reg_device_form(f, xyz_dev, n, true, cols, sys_dev, counts_dev, regn_kernels(f->ctx, c, n));
}

}  // extern "C"
