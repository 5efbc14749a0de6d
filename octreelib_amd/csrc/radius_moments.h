// The moments of the stored points within a radius of a point: the sink of octl_forest_neighbourhood_stats and
// octl_forest_point_stats for the walk of nearest_walk.h, and the row both kernels write (moments.hip states the
// definition, DESIGN.md 4.23 the bound).  __host__ __device__, so that a stand-alone host program runs the very code
// of the kernels (tests/host/moments_host.cpp: a CPU build under the sanitizers, compared with
// neighbourhood_statistics_np).
#pragma once
#include "leaf_moments.h"
#include "nearest_walk.h"
#include "sym3_eigen.h"

// worst() is always +inf: nothing prunes below r2, and every stored point with d2 <= r2 is offered - the candidates of
// octl_forest_radius_count, uncapped.  offer counts the point and adds it to the nine shifted sums of leaf_moments.h:
// Sums, taken relative to the query: dx = fl(p_x - q_x) - the walk's own difference with the sign turned, which is
// exact - then s += dx and s = fma(dx, dy, s), in f64, one point after the other in the order of the walk.  Every
// term is bounded by the radius whatever the magnitude of the coordinates.  The point is read again from the ordered
// arrays (pos is its row): the walk hands a sink no coordinates, and the row is in the cache it has just come through.
struct RadiusMoments {
  const double* xyz_ord;
  double qx, qy, qz;
  int64_t n;
  Sums S;
  __host__ __device__ __forceinline__ void clear() {
    n = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) S.s[k] = 0.0;
  }
  __host__ __device__ __forceinline__ double worst() const { return nn_infinity(); }
  __host__ __device__ __forceinline__ void offer(double, uint64_t, uint32_t pos) {
    const double* __restrict__ p = xyz_ord + 3 * (int64_t)pos;
    const double dx = p[0] - qx, dy = p[1] - qy, dz = p[2] - qz;
    n += 1;
    S.s[0] += dx;
    S.s[1] += dy;
    S.s[2] += dz;
    S.s[3] = fma(dx, dx, S.s[3]);
    S.s[4] = fma(dx, dy, S.s[4]);
    S.s[5] = fma(dx, dz, S.s[5]);
    S.s[6] = fma(dy, dy, S.s[6]);
    S.s[7] = fma(dy, dz, S.s[7]);
    S.s[8] = fma(dz, dz, S.s[8]);
  }
};

// One row: the walk, then finish() of leaf_moments.h with p0 = q, then - eigval != nullptr - the Jacobi solver of
// sym3_eigen.h.  Returns the count; mean[3], cov[6] (xx xy xz yy yz zz), eigval[3], eigvec[9].  A row without a
// neighbour (no stored point within the radius, a query that is not finite, a forest without roots) is NaN in every
// field but the count.  A single neighbour has no spread: its covariance is written as exact zeros instead of the
// rounding residue fl(dx dx) - dx dx of the one-pass form, so that its eigenvalues are zeros too.
__host__ __device__ __forceinline__ int64_t moments_row(const NNTables& T, double qx, double qy, double qz, double r,
                                                        double r2, double* mean, double* cov, double* eigval,
                                                        double* eigvec) {
  RadiusMoments m;
  m.xyz_ord = T.xyz_ord;
  m.qx = qx, m.qy = qy, m.qz = qz;
  m.clear();
  nearest_walk(T, qx, qy, qz, r, r2, m);
  double c6[6];
  if (m.n > 0) {
    finish(m.S, m.n, qx, qy, qz, mean, c6);
    if (m.n == 1)
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = 0.0;
  } else {
    const double nan = nn_infinity() - nn_infinity();
    mean[0] = mean[1] = mean[2] = nan;
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = nan;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) cov[k] = c6[k];
  if (eigval) {
    double w[3], v[9];
    sym3_eigen(c6, w, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) eigval[k] = w[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) eigvec[k] = v[k];
  }
  return m.n;
}
