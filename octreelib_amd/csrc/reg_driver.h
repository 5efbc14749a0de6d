// The host side the three scan-to-map registration systems share (register.hip, register_points.hip,
// register_nearest_plane.hip): the scratch of a call, the check of the transform, the fold's launch and the two forms
// every system comes in.  A system lists its per-point columns (all given or none) and hands a form the callable that
// enqueues its own kernels:  int launch(const double* xyz_dev, void* const* col_dev, const RegScratch& s,
// double* sys_dev, int64_t* counts_dev),  col_dev[k] the device array of column k (nullptr: not asked for).
//   host form    n = 0: host zeros.  Otherwise f->q_stage holds [queries 3 f64 | the columns in their order, when asked
//                for], reserved BEFORE the scratch; one upload, the kernels, the download of the 28 + 2 numbers through
//                the pinned mirror and of the columns, ONE host wait.
//   device form  n = 0: two fills in stream order.  Otherwise the scratch, the stream's wait for the scan's upload, the
//                kernels; the host does not wait.
// What a system refuses is its own *_begin's business and comes before either form: they reserve and enqueue.
#pragma once
#include <cmath>

#include "common.h"
#include "forest.h"
#include "reg_fold.h"

namespace {

// scratch of one call in f->rg_rows: [0, 256) the result (28 sums, 2 counts), the rows, then the 32-byte records of
// the systems that match before they sum
struct RegScratch {
  double *result, *rows;
  double4* rec;
};

int reg_scratch(octl_forest* f, int64_t n, bool with_records, RegScratch* s) {
  const size_t rows_bytes = (size_t)ceil_div(n, RS_CHUNK) * RS_ROW * 8;
  OCTL_TRY(devbuf_reserve(f->ctx, f->rg_rows, 256 + rows_bytes + (with_records ? (size_t)n * 32 : 0)));
  char* base = static_cast<char*>(f->rg_rows.p);
  s->result = reinterpret_cast<double*>(base);
  s->rows = reinterpret_cast<double*>(base + 256);
  s->rec = reinterpret_cast<double4*>(base + 256 + rows_bytes);
  return OCTL_OK;
}

int reg_check_transform(octl_ctx* ctx, const char* what, const double* T, const double* origin) {
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(T[k])) return octl_set_error(ctx, OCTL_E_INVALID, "%s: the transform is not finite", what);
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k])) return octl_set_error(ctx, OCTL_E_INVALID, "%s: the origin is not finite", what);
  return OCTL_OK;
}

// one per-point answer: the caller's array (host form: in host memory, device form: in device memory) and its element
struct RegColumn {
  void* p;
  size_t elem;
};

template <size_t NC>
bool reg_columns_ok(const RegColumn (&cols)[NC]) {
  size_t given = 0;
  for (const RegColumn& c : cols) given += c.p ? 1 : 0;
  return given == 0 || given == NC;
}

int reg_fold_launch(octl_ctx* ctx, const double* rows, int64_t n_rows, double* sys_dev, int64_t* counts_dev) {
  KTimer timer(ctx, "reg_fold");
  OCTL_LAUNCH(k_reg_fold, dim3(1), dim3(256), 0, ctx->stream, rows, n_rows, sys_dev, counts_dev);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

template <size_t NC, class Launch>
int reg_host_form(octl_forest* f, const double* xyz, int64_t n, bool with_records, const RegColumn (&cols)[NC],
                  double* sys, int64_t* counts, Launch&& launch) {
  if (n == 0) {
    for (int k = 0; k < RS_SUMS; ++k) sys[k] = 0.0;
    counts[0] = counts[1] = 0;
    return OCTL_OK;
  }
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const bool asked = cols[0].p != nullptr;
  Carve plan;
  const auto q_part = plan.add<double>((size_t)n * 3);
  Carve::Part<char> part[NC];
  if (asked)
    for (size_t k = 0; k < NC; ++k) part[k] = plan.add<char>((size_t)n * cols[k].elem);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, plan.total));
  RegScratch s;
  OCTL_TRY(reg_scratch(f, n, with_records, &s));
  double* q_d = Carve::at(f->q_stage, q_part);
  void* col_d[NC] = {};
  if (asked)
    for (size_t k = 0; k < NC; ++k) col_d[k] = Carve::at(f->q_stage, part[k]);
  HIP_TRY(ctx, hipMemcpyAsync(q_d, xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OCTL_TRY(launch(q_d, col_d, s, s.result, reinterpret_cast<int64_t*>(s.result + RS_SUMS)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->small_host, s.result, (RS_SUMS + 2) * 8, hipMemcpyDeviceToHost, st));
  if (asked)
    for (size_t k = 0; k < NC; ++k)
      HIP_TRY(ctx, hipMemcpyAsync(cols[k].p, col_d[k], (size_t)n * cols[k].elem, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memcpy(sys, ctx->small_host, RS_SUMS * 8);
  std::memcpy(counts, static_cast<const char*>(ctx->small_host) + RS_SUMS * 8, 16);
  return OCTL_OK;
}

template <size_t NC, class Launch>
int reg_device_form(octl_forest* f, const double* xyz_dev, int64_t n, bool with_records, const RegColumn (&cols)[NC],
                    double* sys_dev, int64_t* counts_dev, Launch&& launch) {
  octl_ctx* ctx = f->ctx;
  if (n == 0) {  // (nothing to reduce: the zeros are two fills in stream order)
    HIP_TRY(ctx, hipMemsetAsync(sys_dev, 0, RS_SUMS * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(counts_dev, 0, 16, ctx->stream));
    return OCTL_OK;
  }
  RegScratch s;
  OCTL_TRY(reg_scratch(f, n, with_records, &s));
  OCTL_TRY(ctx_wait_uploads(ctx, xyz_dev, (size_t)n * 24));
  void* col_d[NC];
  for (size_t k = 0; k < NC; ++k) col_d[k] = cols[k].p;
  return launch(xyz_dev, col_d, s, sys_dev, counts_dev);
}

}  // namespace
