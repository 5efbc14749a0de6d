// Ray evidence per leaf: octl_forest_ray_evidence.  For every leaf of the scheme, how many rays END in
// it and how many only pass THROUGH it - what a map needs to find the leaves that later scans saw through (free-space
// evidence; octl_forest_carve in mask.hip removes what they hold).  Defined by the brute force over the leaves of
// octreelib_amd/query.py: ray_evidence_np and compared with it for equality.  No reference counterpart: the reference
// has no ray query.
//
//   per ray o, d, t_min, t_free, t_end:  F = [t_min, t_free] (empty when t_free < t_min), E = [e0, t_end] with e0 =
//   max(t_min, t_free) (empty when t_end < e0); dead as a ray of octl_forest_raycast is (t_free and t_end both finite);
//   per leaf: near, far and the pass test of raycast's interval (raycast.hip), near = max over the bounding axes,
//   far = min;  in_E iff every axis passes and max(near, e0) <= min(far, t_end);  in_F iff every axis passes and
//   max(near, t_min) <= min(far, t_free);  hits[leaf] = rays with in_E, through[leaf] = rays with in_F and not in_E.
//   Inner nodes hold 0.
//   The scheme and the rays alone decide: no occupancy, no pose selection.
//
// One kernel per call, one ray per lane, grid-stride, no LDS, no scratch: raycast_walk.h's march and stackless descent
// over [t_min, max(t_free, t_end)] with nothing pruned by a best t, one u32 atomicAdd per crossed leaf.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "forest.h"
#include "query_walk.h"
#include "raycast_walk.h"

namespace {

__global__ __launch_bounds__(256) void k_ray_evidence(const double* __restrict__ org, const double* __restrict__ dir,
                                                      const double* __restrict__ t_min,
                                                      const double* __restrict__ t_free,
                                                      const double* __restrict__ t_end, int64_t n, EvidenceTables T) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    ray_evidence(T, org + 3 * i, dir + 3 * i, t_min[i], t_free[i], t_end[i]);
}

int launch_evidence(octl_ctx* ctx, const double* org, const double* dir, const double* t_min, const double* t_free,
                    const double* t_end, int64_t n, const EvidenceTables& T) {
  KTimer timer(ctx, "ray_evidence");
  const unsigned wgs = grid_stride_for(ctx, n);
  OCTL_LAUNCH(k_ray_evidence, dim3(wgs), dim3(256), 0, ctx->stream, org, dir, t_min, t_free, t_end, n, T);
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

// host form: a ray whose t are finite and whose walk is not empty must respect the grid's cap, as a ray of raycast
int evidence_check_cap(octl_forest* f, const double* t_min, const double* t_free, const double* t_end, int64_t n) {
  if (f->mode != 0) return OCTL_OK;
  const double span = RAY_CAP_EDGES * f->edge, lim = RAY_T_LIMIT * f->edge;
  for (int64_t i = 0; i < n; ++i) {
    const double a = t_min[i];
    if (!(std::isfinite(a) && std::isfinite(t_free[i]) && std::isfinite(t_end[i]))) continue;
    const double b = std::fmax(t_free[i], t_end[i]);
    if (!(a <= b)) continue;
    if (!(b - a <= span))
      return octl_set_error(f->ctx, OCTL_E_INVALID,
                            "ray_evidence: ray %lld spans max(t_free, t_end) - t_min = %g, more than %g voxel edges "
                            "of %g (the cap bounds a call's cost)",
                            (long long)i, b - a, RAY_CAP_EDGES, f->edge);
    if (!(std::fabs(a) <= lim && std::fabs(b) <= lim))
      return octl_set_error(f->ctx, OCTL_E_INVALID, "ray_evidence: ray %lld has |t| above 2^40 voxel edges of %g",
                            (long long)i, f->edge);
  }
  return OCTL_OK;
}

// what both forms start with: the refusals and the tables (the scheme alone: nothing is made, nothing can be stale)
int evidence_begin(octl_forest* f, int64_t n, bool pointers_ok, EvidenceTables* T) {
  OCTL_TRY(query_begin(f, "ray_evidence", &T->t));
  if (query_bad_count(n) || !pointers_ok)
    return octl_set_error(f->ctx, OCTL_E_INVALID, "bad ray_evidence arguments");
  const NodeTable& nt = f->nodes[f->cur];
  T->parent = nt.parent.as<int32_t>();
  T->max_steps = 4 * nt.n + 64;
  T->through = T->hits = nullptr;
  return OCTL_OK;
}

}  // namespace

extern "C" {

int octl_forest_ray_evidence(octl_forest* f, const double* origins, const double* directions, const double* t_min,
                             const double* t_free, const double* t_end, int64_t n, int64_t cap_nodes,
                             uint32_t* through, uint32_t* hits, int64_t* n_nodes) {
  if (!f || !n_nodes) return OCTL_E_INVALID;
  EvidenceTables T;
  OCTL_TRY(evidence_begin(f, n, n <= 0 || (origins && directions && t_min && t_free && t_end), &T));
  octl_ctx* ctx = f->ctx;
  const int64_t N = f->nodes[f->cur].n;
  *n_nodes = N;
  if (cap_nodes < N || N == 0) return OCTL_OK;  // (the size query: cap_nodes = 0)
  if (!through || !hits) return octl_set_error(ctx, OCTL_E_INVALID, "bad ray_evidence arguments");
  if (n == 0) {
    std::fill(through, through + N, 0u);
    std::fill(hits, hits + N, 0u);
    return OCTL_OK;
  }
  OCTL_TRY(evidence_check_cap(f, t_min, t_free, t_end, n));
  // one upload per input, one fill of both counters, the kernel, a download per counter array, one wait
  hipStream_t st = ctx->stream;
  Carve plan;  // f->q_stage: [through u32 N, hits u32 N | origins 3 f64 | directions 3 f64 | t_min | t_free | t_end]
  const auto c_part = plan.add<uint32_t>((size_t)N * 2);
  const auto o_part = plan.add<double>((size_t)n * 3), d_part = plan.add<double>((size_t)n * 3);
  const auto a_part = plan.add<double>((size_t)n), b_part = plan.add<double>((size_t)n);
  const auto e_part = plan.add<double>((size_t)n);
  OCTL_TRY(devbuf_reserve(ctx, f->q_stage, plan.total));
  uint32_t* c_d = Carve::at(f->q_stage, c_part);
  double *o_d = Carve::at(f->q_stage, o_part), *d_d = Carve::at(f->q_stage, d_part);
  double *a_d = Carve::at(f->q_stage, a_part), *b_d = Carve::at(f->q_stage, b_part);
  double* e_d = Carve::at(f->q_stage, e_part);
  HIP_TRY(ctx, hipMemcpyAsync(o_d, origins, (size_t)n * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_d, directions, (size_t)n * 24, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(a_d, t_min, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(b_d, t_free, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(e_d, t_end, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(c_d, 0, (size_t)N * 8, st));
  T.through = c_d;
  T.hits = c_d + N;
  OCTL_TRY(launch_evidence(ctx, o_d, d_d, a_d, b_d, e_d, n, T));
  HIP_TRY(ctx, hipMemcpyAsync(through, c_d, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hits, c_d + N, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return OCTL_OK;
}

int octl_forest_ray_evidence_device(octl_forest* f, const double* origins_dev, const double* directions_dev,
                                    const double* t_min_dev, const double* t_free_dev, const double* t_end_dev,
                                    int64_t n, uint32_t* through_dev, uint32_t* hits_dev, int64_t n_nodes) {
  if (!f) return OCTL_E_INVALID;
  EvidenceTables T;
  const bool pointers_ok = n <= 0 || (origins_dev && directions_dev && t_min_dev && t_free_dev && t_end_dev &&
                                      through_dev && hits_dev);
  OCTL_TRY(evidence_begin(f, n, pointers_ok, &T));
  octl_ctx* ctx = f->ctx;
  const int64_t N = f->nodes[f->cur].n;
  if (n_nodes != N)
    return octl_set_error(ctx, OCTL_E_INVALID, "ray_evidence: counters for %lld nodes, the scheme has %lld",
                          (long long)n_nodes, (long long)N);
  if (n == 0) return OCTL_OK;
  // (any of the inputs may be the target of an octl_dev_upload_async that is still in flight: ordered on the device)
  OCTL_TRY(ctx_wait_uploads(ctx, origins_dev, (size_t)n * 24));
  OCTL_TRY(ctx_wait_uploads(ctx, directions_dev, (size_t)n * 24));
  OCTL_TRY(ctx_wait_uploads(ctx, t_min_dev, (size_t)n * 8));
  OCTL_TRY(ctx_wait_uploads(ctx, t_free_dev, (size_t)n * 8));
  OCTL_TRY(ctx_wait_uploads(ctx, t_end_dev, (size_t)n * 8));
  OCTL_TRY(ctx_wait_uploads(ctx, through_dev, (size_t)N * 4));
  OCTL_TRY(ctx_wait_uploads(ctx, hits_dev, (size_t)N * 4));
  T.through = through_dev;
  T.hits = hits_dev;
  return launch_evidence(ctx, origins_dev, directions_dev, t_min_dev, t_free_dev, t_end_dev, n, T);
}

}  // extern "C"
