// One matched point of the point-to-point registration system (octl_forest_point_registration_system,
// register_points.hip: k_regp_partial): its contribution to the 17 distinct sums of the 6x6 system,
// and the expansion of those 17 into the 28-number layout of registration.system_from_sums.  __host__ __device__, so
// that a stand-alone host program runs the very code of the kernel (tests/host/point_term_host.cpp) and a Fraction
// emulation of the order below can be compared with it bit for bit.
//
// Inputs: the transformed point p, the origin c, e = fl(p - m) per component and d2 - the bits the search formed -,
// delta (<= 0: no Huber weights) and delta2 = fl(delta delta).  Every operation is one IEEE f64 operation, none is
// contracted (the library is built with -ffp-contract=off); `fma(a, b, c)` is ONE rounding of the exact a b + c.
//
//   d_i  = p_i - c_i                                           3 plain subtractions
//   tail = delta > 0 and d2 > delta2                           (decided on d2: both sides branch on the same bits)
//   w    = tail ? delta / sqrt(d2) : 1                         s = sqrt(d2), then one division
//   wd_i = w d_i,  we_i = w e_i                                6 plain products (exact when w = 1)
//   S[0] += fma(wd_y, d_y, wd_z d_z)      H_ww(0,0)            one plain product, one fma, one plain addition
//   S[1] += fma(wd_x, d_x, wd_z d_z)      H_ww(1,1)            (each product wd_i d_i is formed once)
//   S[2] += fma(wd_x, d_x, wd_y d_y)      H_ww(2,2)
//   S[3]  = fma(-wd_x, d_y, S[3])         H_ww(0,1)            the product enters the sum through the fma
//   S[4]  = fma(-wd_x, d_z, S[4])         H_ww(0,2)
//   S[5]  = fma(-wd_y, d_z, S[5])         H_ww(1,2)
//   S[6..8]  += wd_x, wd_y, wd_z          H_wv = [sum w d]x    plain additions
//   S[9]     += w                         H_vv = (sum w) I
//   S[10] += fma(wd_y, e_z, -(wd_z e_y))  g_w = sum w d x e    one plain product (negated: exact), one fma, one
//   S[11] += fma(wd_z, e_x, -(wd_x e_z))                       plain addition
//   S[12] += fma(wd_x, e_y, -(wd_y e_x))
//   S[13..15] += we_x, we_y, we_z         g_v = sum w e        plain additions
//   S[16] += tail ? delta (s - 0.5 delta) : 0.5 d2             the cost: rho (0.5 x is exact)
//
// Roundings of a term before the addition that enters it into its sum, relative to the absolute values of the products
// it is made of: H_ww diagonal 7 (d twice, sqrt, division, w d, the product, the fma), H_ww off-diagonal 5, H_wv 4,
// H_vv 2, g_w 6, g_v 3, cost 4 (s - delta / 2 >= s / 2 doubles the error of s) - at most 7.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

constexpr int RP_SUMS = 17;

__host__ __device__ __forceinline__ void reg_point_term(const double p[3], const double c[3], const double e[3],
                                                        double d2, double delta, double delta2, double S[RP_SUMS]) {
  const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
  const bool tail = delta > 0.0 && d2 > delta2;
  double w = 1.0, rho = 0.5 * d2;
  if (tail) {
    const double s = sqrt(d2);
    w = delta / s;
    rho = delta * (s - 0.5 * delta);
  }
  const double wdx = w * dx, wdy = w * dy, wdz = w * dz;
  const double wex = w * e[0], wey = w * e[1], wez = w * e[2];
  const double yy = wdy * dy, zz = wdz * dz;
  S[0] += fma(wdy, dy, zz);
  S[1] += fma(wdx, dx, zz);
  S[2] += fma(wdx, dx, yy);
  S[3] = fma(-wdx, dy, S[3]);
  S[4] = fma(-wdx, dz, S[4]);
  S[5] = fma(-wdy, dz, S[5]);
  S[6] += wdx;
  S[7] += wdy;
  S[8] += wdz;
  S[9] += w;
  S[10] += fma(wdy, e[2], -(wdz * e[1]));
  S[11] += fma(wdz, e[0], -(wdx * e[2]));
  S[12] += fma(wdx, e[1], -(wdy * e[0]));
  S[13] += wex;
  S[14] += wey;
  S[15] += wez;
  S[16] += rho;
}

// The 28 numbers of registration.system_from_sums (21 of H's upper triangle row-major, 6 of g, the cost) from the 17:
// copies, sign changes (0 - x: exact, and +0 for x = 0) and structural zeros (+0) alone.
//   H_wv = [sum w d]x = ( 0 -z  y ; z  0 -x ; -y  x  0 ),  H_vv = (sum w) I
__host__ __device__ __forceinline__ void reg_point_expand(const double S[RP_SUMS], double out[28]) {
  const double X = S[6], Y = S[7], Z = S[8], W = S[9];
  const double row[28] = {S[0], S[3], S[4], 0.0,     0.0 - Z, Y,        // H row 0
                          S[1], S[5], Z,    0.0,     0.0 - X,           // H row 1
                          S[2], 0.0 - Y,    X,       0.0,               // H row 2
                          W,    0.0,        0.0,                        // H rows 3 - 5
                          W,    0.0,                                    //
                          W,                                            //
                          S[10], S[11], S[12], S[13], S[14], S[15],     // g
                          S[16]};                                       // cost
#pragma unroll
  for (int k = 0; k < 28; ++k) out[k] = row[k];
}
