// Point-to-point scan-to-map registration, the device's share: for ONE rigid transform T the normal equations of a
// scan against the nearest stored point of every transformed query (octl_forest_point_registration_system, DESIGN.md
// 4.19) - classic ICP where the map has no planes to offer.  The 6x6 solve, the pose update and the loop stay on the
// host (octreelib_amd/registration.py: point_registration_system_np is the definition, align_np the loop).  No
// reference counterpart: the reference has no registration.
//
// Per query q:
//   p = ((R_i0 q_x + R_i1 q_y) + R_i2 q_z) + t_i, every product and sum rounded (the bits of transform_np);
//   the nearest stored point m of the selection within max_distance: the search of octl_forest_nearest with k = 1
//   (nearest_walk.h - the same cubes, the same d2 bits, the same total order (d2, slot, index));
//   used iff there is one; e = fl(p - m), d2 as the search formed it;
//   the point's term of the 17 distinct sums: reg_point_term.h, which fixes the operation order.
//
// Three launches in stream order:
//   k_reg_match    one query per lane, grid-stride, launched as k_nearest is: writes one 32-byte record {e, d2} per
//                  query (d2 = +inf: unused) and, in its second instance, slot / index / distance2;
//   k_regp_partial the summation tree of k_reg_partial unchanged (register.hip): chunks of 4096, lane tid takes
//                  4096 k + 256 j + tid for j = 0..15 in that order, the 17 sums expanded to the 28-number row by
//                  copies and sign changes, reg_block_reduce, row k.  No walk: 56 bytes per query streamed;
//   k_reg_fold     as it is (reg_fold.h).
// The tree is a function of n alone: no floating-point atomics, nothing sized by the CU count (the grid of k_reg_match
// is, and it adds nothing).  The host and the device form around the launches: reg_driver.h.  LDS: 960 bytes
// (k_regp_partial, k_reg_fold), none in k_reg_match.
#include "common.h"
#include "forest.h"
#include "nearest_walk.h"
#include "reg_best.h"
#include "reg_driver.h"
#include "reg_fold.h"
#include "reg_point_term.h"

namespace {

struct RegPointParams {
  double T[12];  // row-major 3 x 4: R | t
  double c[3];   // origin of the rotational part
  double delta;  // <= 0: no weights
  double delta2;
};

// (RegBest, the k = 1 sink: reg_best.h; reg_transform: reg_fold.h - register_nearest_plane.hip matches with the same)

template <bool PER_POINT>
__global__ __launch_bounds__(256) void k_reg_match(const double* __restrict__ xyz, int64_t n, RegPointParams P, double r,
                                                   double r2, NNTables T, double4* __restrict__ rec_out,
                                                   int32_t* __restrict__ slot_out, int64_t* __restrict__ index_out,
                                                   double* __restrict__ d2_out) {
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double p[3];
    reg_transform(P.T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], p);
    RegBest best = {INF, ~0ull, 0u};
    nearest_walk(T, p[0], p[1], p[2], r, r2, best);
    const bool has = best.bid != ~0ull;
    double4 rec = make_double4(0.0, 0.0, 0.0, INF);
    if (has) {
      // (the operands and the operation of the walk's own dx, dy, dz: the same bits)
      const double* __restrict__ m = T.xyz_ord + 3 * (int64_t)best.pos;
      rec = make_double4(p[0] - m[0], p[1] - m[1], p[2] - m[2], best.bd);
    }
    rec_out[i] = rec;
    if (PER_POINT) {
      slot_out[i] = has ? (int32_t)(best.bid >> 32) : -1;
      index_out[i] = has ? (int64_t)(best.bid & 0xffffffffull) : -1;
      d2_out[i] = best.bd;
    }
  }
}

__global__ __launch_bounds__(256) void k_regp_partial(const double* __restrict__ xyz, int64_t n, RegPointParams P,
                                                      const double4* __restrict__ rec, double* __restrict__ rows) {
  __shared__ double lds[4][RS_SUMS];
  __shared__ long long ldc[4][2];
  const double INF = __longlong_as_double(0x7ff0000000000000ll);
  double S[RP_SUMS];
#pragma unroll
  for (int k = 0; k < RP_SUMS; ++k) S[k] = 0.0;
  long long used = 0, located = 0;
  const int64_t base = (int64_t)blockIdx.x * RS_CHUNK + threadIdx.x;
#pragma unroll 1
  for (int j = 0; j < RS_CHUNK / 256; ++j) {
    const int64_t i = base + (int64_t)j * 256;
    if (i >= n) break;
    double p[3];
    reg_transform(P.T, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], p);
    located += (fabs(p[0]) < INF && fabs(p[1]) < INF && fabs(p[2]) < INF) ? 1 : 0;  // (false for NaN)
    const double4 m = rec[i];
    if (!(m.w < INF)) continue;  // (no match: skipped, never multiplied by zero)
    used += 1;
    const double e[3] = {m.x, m.y, m.z};
    reg_point_term(p, P.c, e, m.w, P.delta, P.delta2, S);
  }
  RegAcc a;
  reg_point_expand(S, a.s);
  a.used = used;
  a.located = located;
  reg_block_reduce(a, lds, ldc);
  reg_write_row(a, rows);
}

struct RegPointCall {
  RegPointParams P;
  NNTables T;
  double r;
};

const char* const WHAT = "point_registration_system";

// the checks every form starts with (nothing has run when one of them fails): the search's, then the system's
int regp_begin(octl_forest* f, const void* xyz, int64_t n, const double* T, const double* origin, double max_distance,
               double huber_delta, const uint8_t* slot_sel, int32_t n_sel, const void* sys, const void* counts,
               bool columns_ok, RegPointCall* c) {
  const bool pointers_ok = (n <= 0 || xyz) && T && origin && sys && counts && columns_ok;
  octl_ctx* ctx = f->ctx;
  // (nearest_begin ends by making the block index: what the system refuses comes first.  Before build, and with
  //  pointers missing, nearest_begin itself refuses - state, then arguments)
  if (f->built && pointers_ok) OCTL_TRY(reg_check_transform(ctx, WHAT, T, origin));
  OCTL_TRY(nearest_begin(f, WHAT, n, 1, max_distance, slot_sel, n_sel, pointers_ok, &c->T));
  std::memcpy(c->P.T, T, sizeof c->P.T);
  std::memcpy(c->P.c, origin, sizeof c->P.c);
  c->P.delta = huber_delta > 0.0 ? huber_delta : 0.0;
  c->P.delta2 = c->P.delta * c->P.delta;
  c->r = max_distance;
  return OCTL_OK;
}

// the three kernels of a call, as the forms of reg_driver.h enqueue them; columns: slot, index, distance2
auto regp_kernels(octl_ctx* ctx, const RegPointCall& c, int64_t n) {
  return [ctx, &c, n](const double* xyz_dev, void* const* col, const RegScratch& s, double* sys_dev,
                      int64_t* counts_dev) -> int {
    const int64_t n_rows = ceil_div(n, RS_CHUNK);
    const double r2 = c.r * c.r;
    {
      KTimer timer(ctx, "reg_match");
      const unsigned wgs = grid_stride_for(ctx, n);
      if (col[0])
        OCTL_LAUNCH(k_reg_match<true>, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.r, r2, c.T, s.rec,
                    (int32_t*)col[0], (int64_t*)col[1], (double*)col[2]);
      else
        OCTL_LAUNCH(k_reg_match<false>, dim3(wgs), dim3(256), 0, ctx->stream, xyz_dev, n, c.P, c.r, r2, c.T, s.rec,
                    nullptr, nullptr, nullptr);
      HIP_TRY(ctx, hipGetLastError());
    }
    {
      KTimer timer(ctx, "regp_partial");
      OCTL_LAUNCH(k_regp_partial, dim3((unsigned)n_rows), dim3(256), 0, ctx->stream, xyz_dev, n, c.P,
                  (const double4*)s.rec, s.rows);
      HIP_TRY(ctx, hipGetLastError());
    }
    return reg_fold_launch(ctx, s.rows, n_rows, sys_dev, counts_dev);
  };
}

}  // namespace

extern "C" {

int octl_forest_point_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                          const double origin[3], double max_distance, double huber_delta,
                                          const uint8_t* slot_sel, int32_t n_sel, double sys[28], int64_t counts[2],
                                          int32_t* slot, int64_t* index, double* distance2) {
  if (!f) return OCTL_E_INVALID;
  RegPointCall c;
  const RegColumn cols[] = {{slot, 4}, {index, 8}, {distance2, 8}};
  OCTL_TRY(regp_begin(f, xyz, n, T, origin, max_distance, huber_delta, slot_sel, n_sel, sys, counts,
                      reg_columns_ok(cols), &c));
  return reg_host_form(f, xyz, n, true, cols, sys, counts, regp_kernels(f->ctx, c, n));
}

int octl_forest_point_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n, const double T[12],
                                                 const double origin[3], double max_distance, double huber_delta,
                                                 const uint8_t* slot_sel, int32_t n_sel, double* sys_dev,
                                                 int64_t* counts_dev, int32_t* slot_dev, int64_t* index_dev,
                                                 double* distance2_dev) {
  if (!f) return OCTL_E_INVALID;
  RegPointCall c;
  const RegColumn cols[] = {{slot_dev, 4}, {index_dev, 8}, {distance2_dev, 8}};
  OCTL_TRY(regp_begin(f, xyz_dev, n, T, origin, max_distance, huber_delta, slot_sel, n_sel, sys_dev, counts_dev,
                      reg_columns_ok(cols), &c));
  return reg_device_form(f, xyz_dev, n, true, cols, sys_dev, counts_dev, regp_kernels(f->ctx, c, n));
}

}  // extern "C"
