// One used point of a point-to-plane registration system: its contribution to the 28 sums of the 6x6 system (21 of
// H's upper triangle row-major, 6 of g, the cost).  Shared by register.hip (k_reg_partial: the plane of the point's own
// leaf) and register_nearest_plane.hip (k_regn_partial: the plane of the nearest stored point's leaf,
// DESIGN.md 4.21) - one definition, so that both enter a term with the same operations in the same order.
// __host__ __device__, as reg_point_term.h is.
//
// Inputs: the transformed point p, the origin c, the plane's unit normal n, the residual r and ar = |r| (finite),
// delta (<= 0: no Huber weights).  Every operation is one IEEE f64 operation, none is contracted (the library is built
// with -ffp-contract=off); `fma(a, b, c)` is ONE rounding of the exact a b + c.
//
//   d_i  = p_i - c_i                                           3 plain subtractions
//   J    = [d x n, n]                                          one plain product (negated: exact) and one fma each
//   tail = delta > 0 and ar > delta;  w = tail ? delta / ar : 1
//   wj_u = w J_u                                               6 plain products (exact when w = 1)
//   s[k(u, v)] = fma(wj_u, J_v, s[k(u, v)]),  u <= v           the product enters the sum through the fma
//   s[21 + u]  = fma(wj_u, r, s[21 + u])
//   s[27]     += delta (ar - 0.5 delta)            (tail)      the cost: rho
//   s[27]      = fma(0.5 r, r, s[27])              (otherwise; 0.5 r is exact)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

__host__ __device__ __forceinline__ void reg_plane_term(double px, double py, double pz, const double c[3],
                                                        const double nrm[3], double r, double ar, double huber_delta,
                                                        double s[28]) {
  const double dx = px - c[0], dy = py - c[1], dz = pz - c[2];
  double J[6];
  J[0] = fma(dy, nrm[2], -(dz * nrm[1]));
  J[1] = fma(dz, nrm[0], -(dx * nrm[2]));
  J[2] = fma(dx, nrm[1], -(dy * nrm[0]));
  J[3] = nrm[0];
  J[4] = nrm[1];
  J[5] = nrm[2];
  const bool tail = huber_delta > 0.0 && ar > huber_delta;
  const double w = tail ? huber_delta / ar : 1.0;
  int k = 0;
#pragma unroll
  for (int u = 0; u < 6; ++u) {
    const double wj = w * J[u];
#pragma unroll
    for (int v = u; v < 6; ++v, ++k) s[k] = fma(wj, J[v], s[k]);
    s[21 + u] = fma(wj, r, s[21 + u]);
  }
  if (tail)
    s[27] += huber_delta * (ar - 0.5 * huber_delta);
  else
    s[27] = fma(0.5 * r, r, s[27]);
}
