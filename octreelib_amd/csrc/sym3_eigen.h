// Eigen-decomposition of a symmetric 3x3 matrix in f64 by cyclic Jacobi (leaf_stats.hip: k_leaf_eigen,
// octl_debug_sym3_eigen).  Everything lives in scalars: no arrays, so nothing is indexed dynamically and nothing
// spills.  Host-callable as well, so that the solver can be exercised without a device.
//
// Contract: eigenvalues ascending (ties keep Jacobi's column order: a diagonal matrix keeps its identity columns),
// eigenvectors as the columns of a row-major 3x3, each oriented so that its largest-magnitude component is positive
// (on equal magnitudes the lowest index).  The matrix is first scaled by the power of two at or above its largest
// entry - exact, so entries from 1e-150 to 1e150 neither overflow nor underflow in the rotations.  A rotation is
// skipped (its off-diagonal entry set to zero) once that entry is below 2^-60 of the scaled matrix's largest entry,
// which changes no eigenvalue by more than 2^-60 * max|a|, far below the rounding of the rotations themselves.
// The closed-form (trigonometric) 3x3 solver is deliberately not used: in the planar case - the one that matters
// here - it loses the smallest eigenvalue's vector entirely.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#define SYM3_MAX_SWEEPS 12

// one Jacobi rotation zeroing a_pq (r = the third index): A' = P^T A P, V' = V P (Numerical Recipes' form)
__host__ __device__ __forceinline__ void sym3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                                     double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                                                     double& v2q) {
  if (fabs(apq) <= 0x1p-60) {  // (scaled matrix: max |a| in [0.5, 1))
    apq = 0.0;
    return;
  }
  const double theta = (aqq - app) / (2.0 * apq);  // |theta| <= 2^61: theta^2 cannot overflow
  double t = 1.0 / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(fma(t, t, 1.0));
  const double s = t * c;
  app = fma(-t, apq, app);
  aqq = fma(t, apq, aqq);
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = fma(c, rp, -s * rq);
  arq = fma(s, rp, c * rq);
  double x = v0p, y = v0q;
  v0p = fma(c, x, -s * y);
  v0q = fma(s, x, c * y);
  x = v1p, y = v1q;
  v1p = fma(c, x, -s * y);
  v1q = fma(s, x, c * y);
  x = v2p, y = v2q;
  v2p = fma(c, x, -s * y);
  v2q = fma(s, x, c * y);
}

__host__ __device__ __forceinline__ void sym3_swap_cols(double& wa, double& wb, double& a0, double& b0, double& a1,
                                                        double& b1, double& a2, double& b2) {
  double t = wa; wa = wb; wb = t;
  t = a0; a0 = b0; b0 = t;
  t = a1; a1 = b1; b1 = t;
  t = a2; a2 = b2; b2 = t;
}

// largest |component| positive, lowest index on ties
__host__ __device__ __forceinline__ void sym3_orient(double& x, double& y, double& z) {
  double m = x;
  if (fabs(y) > fabs(m)) m = y;
  if (fabs(z) > fabs(m)) m = z;
  if (m < 0.0) {
    x = -x;
    y = -y;
    z = -z;
  }
}

// c6 = a00 a01 a02 a11 a12 a22; w[3] ascending; v[9] row-major, columns = eigenvectors
__host__ __device__ __forceinline__ void sym3_eigen(const double* c6, double* w, double* v) {
  double a00 = c6[0], a01 = c6[1], a02 = c6[2], a11 = c6[3], a12 = c6[4], a22 = c6[5];
  double m = fmax(fmax(fmax(fabs(a00), fabs(a01)), fmax(fabs(a02), fabs(a11))), fmax(fabs(a12), fabs(a22)));
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
  int e = 0;
  if (m > 0.0 && m <= 1.79769313486231570815e308) {
    frexp(m, &e);  // m = f * 2^e, f in [0.5, 1)
    a00 = ldexp(a00, -e), a01 = ldexp(a01, -e), a02 = ldexp(a02, -e);
    a11 = ldexp(a11, -e), a12 = ldexp(a12, -e), a22 = ldexp(a22, -e);
    for (int sweep = 0; sweep < SYM3_MAX_SWEEPS; ++sweep) {
      if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
      sym3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0,1), r = 2
      sym3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0,2), r = 1
      sym3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1,2), r = 0
    }
    a00 = ldexp(a00, e), a11 = ldexp(a11, e), a22 = ldexp(a22, e);
  } else if (!(m == 0.0)) {  // a NaN or an infinity: nothing meaningful to return
    a00 = a11 = a22 = m - m;
    v00 = v01 = v02 = v10 = v11 = v12 = v20 = v21 = v22 = m - m;
  }
  // stable ascending sort of the three (value, column) pairs
  if (a00 > a11) sym3_swap_cols(a00, a11, v00, v01, v10, v11, v20, v21);
  if (a11 > a22) sym3_swap_cols(a11, a22, v01, v02, v11, v12, v21, v22);
  if (a00 > a11) sym3_swap_cols(a00, a11, v00, v01, v10, v11, v20, v21);
  sym3_orient(v00, v10, v20);
  sym3_orient(v01, v11, v21);
  sym3_orient(v02, v12, v22);
  w[0] = a00, w[1] = a11, w[2] = a22;
  v[0] = v00, v[1] = v01, v[2] = v02;
  v[3] = v10, v[4] = v11, v[5] = v12;
  v[6] = v20, v[7] = v21, v[8] = v22;
}
