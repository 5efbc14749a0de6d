// "No plane holds m of these points": a certificate from the scatter matrix of a block's points.
//
// k_ransac (ransac.hip) ends a block after its first 64 hypotheses when none of the later ones can reach a higher
// inlier count.  The cheap exact case is a hypothesis that already holds every point.  This header supplies the
// next one: the best count L of the first group is n - 1 or n - 2, and NO plane at all holds n (or n - 1) of the
// block's points within the threshold - so no later hypothesis can count more than L, whatever it samples.
// __host__ __device__, f64, no dependency on the kernel: tests/host/plane_cert_host.cpp runs it on the CPU.
//
// The argument.  Let a plane have the normal a, |a| >= 1 - 2^-22 (the reference's planes are unit normals rounded
// to f32; ransac.hip shows which hypotheses that holds for), and let m points lie within t of it in the sense
// |a . p + d| <= t.  Their Euclidean distances are at most t / (1 - 2^-22), so the sum of their squared distances
// to that plane is at most m t^2 / (1 - 2^-22)^2.  The smallest eigenvalue of the scatter matrix of those m points
// about their centroid,  S = sum (p - c)(p - c)^T,  is the MINIMUM of that sum over all planes (the best plane goes
// through the centroid).  So
//      lambda_min(S) > m t^2 (1 + 2^-20)        =>   no such plane holds these m points.
// lambda_min from below without an eigen-solver: S is positive semi-definite, its two larger eigenvalues have a
// product of at most (tr S / 2)^2, and the product of all three is det S:
//      lambda_min(S) >= 4 det S / (tr S)^2.
// All n points: one test.  n - 1 of n points: a plane that holds n - 1 points leaves out some point j (any j, if it
// holds all n), and the scatter of the others about THEIR centroid is
//      S_j = S - n / (n - 1) q_j q_j^T,     q_j = p_j - c,
// so the test is made for every j with m = n - 1.
//
// Rounding (u = 2^-53).  The caller hands over the nine raw sums  sum r, sum r r^T  of r = p - p_0, p_0 one of the
// block's points, n <= 64, summed in any order.  Because p_0 is in the set, tr S >= |p_0 - c|^2 and the raw second
// moments are bounded by  sum |r|^2 = tr S + n |c - p_0|^2 <= 65 tr S.
//   each raw sum: at most 64 roundings (any summation order) on partial sums <= 65 tr S, the products' own
//       roundings, r itself (one f64 subtraction, relative u - it moves every point by u |r|):
//                                                              |err| <= 64 x 65 u tr S + 2^-45 tr S <= 2^-40 tr S
//   each entry of S (one product of first moments, one division by n, one subtraction; the first moments
//       squared are <= n sum |r|^2 by Cauchy-Schwarz):                               |err| <= 2^-39 tr S
//   each entry of S_j (q_j from the same sums, |q_j|^2 <= tr S, n / (n - 1) <= 2):     |err| <= 2^-38 tr S
//   det (six products of three entries, each entry <= tr S in magnitude, nine roundings):
//       |err| <= 18 (2^-38 tr S) (tr S)^2 (1 + 2^-30) + 2^-49 (tr S)^3 <= 2^-33 (tr S)^3
//   the trace itself:                                                                  |err| <= 2^-36 tr S
// The test subtracts an allowance of 2^-30 (tr S)^3 - eight times the bound - from the determinant, adds
// 2^-32 tr S - sixteen times the bound - to the trace it divides by (both in terms of the FULL block's trace, also
// for S_j, whose own trace may be much smaller), and asks for m t^2 (1 + 2^-10) instead of m t^2 (1 + 2^-20):
//      4 (det - 2^-30 tr^3) > m t^2 (1 + 2^-10) (tr_j + 2^-32 tr)^2.
// (A leaf worth the test has det / tr^3 of 10^-4 and more: the allowance, 10^-9, costs nothing.)
// With det - allowance > 0 the true determinant is positive, so the true matrix - positive semi-definite by
// construction - is positive definite and the eigenvalue bound applies to it.
// Anything NaN, non-positive or outside 2^-200 < tr < 2^200, 2^-100 <= t <= 2^100 fails (no overflow or underflow
// of a third power inside that range).  A failed certificate only means that the caller goes on as if there were
// none.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PLANE_CERT_HD __host__ __device__ inline
#else
#define PLANE_CERT_HD inline
#endif

namespace plane_cert {

struct Scatter {
  double xx, xy, xz, yy, yz, zz;   // S about the centroid
  double cx, cy, cz;               // the centroid, relative to the point the sums are relative to
  double tr;                       // tr S
};

// S and the centroid of n points from their raw sums relative to one of them
PLANE_CERT_HD Scatter scatter_from_sums(int n, double sx, double sy, double sz, double sxx, double sxy, double sxz,
                                        double syy, double syz, double szz) {
  Scatter s;
  const double inv_n = 1.0 / (double)n;
  s.cx = sx * inv_n;
  s.cy = sy * inv_n;
  s.cz = sz * inv_n;
  s.xx = sxx - sx * s.cx;
  s.xy = sxy - sx * s.cy;
  s.xz = sxz - sx * s.cz;
  s.yy = syy - sy * s.cy;
  s.yz = syz - sy * s.cz;
  s.zz = szz - sz * s.cz;
  s.tr = (s.xx + s.yy) + s.zz;
  return s;
}

// 4 (det - allowance) > m t^2 (1 + 2^-10) (trace + slack)^2 for the symmetric matrix given, the allowance and the
// slack in terms of tr_full
PLANE_CERT_HD bool eigen_floor_exceeds(double xx, double xy, double xz, double yy, double yz, double zz,
                                       double tr_full, int m, double t) {
  if (!(tr_full > 0x1p-200 && tr_full < 0x1p200 && t >= 0x1p-100 && t <= 0x1p100 && m >= 1)) return false;
  const double tr = (xx + yy) + zz;
  if (!(tr > 0.0)) return false;
  const double det = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz);
  const double allowance = 0x1p-30 * ((tr_full * tr_full) * tr_full);
  const double trb = tr + 0x1p-32 * tr_full;
  const double lhs = 4.0 * (det - allowance);
  const double rhs = ((double)m * (t * t)) * (1.0 + 0x1p-10) * (trb * trb);
  return lhs > rhs;   // (false for NaN)
}

// no plane with |normal| >= 1 - 2^-22 holds all n points within t
PLANE_CERT_HD bool no_plane_holds_all(const Scatter& s, int n, double t) {
  if (n < 3) return false;
  return eigen_floor_exceeds(s.xx, s.xy, s.xz, s.yy, s.yz, s.zz, s.tr, n, t);
}

// ... holds the n - 1 points other than the one at (rx, ry, rz) (relative like the sums); every point of the
// block has to pass for "no plane holds n - 1 of the n points"
PLANE_CERT_HD bool no_plane_holds_others(const Scatter& s, int n, double rx, double ry, double rz, double t) {
  if (n < 4) return false;
  const double qx = rx - s.cx, qy = ry - s.cy, qz = rz - s.cz;
  const double w = (double)n / (double)(n - 1);
  const double wx = w * qx, wy = w * qy, wz = w * qz;
  return eigen_floor_exceeds(s.xx - wx * qx, s.xy - wx * qy, s.xz - wx * qz, s.yy - wy * qy, s.yz - wy * qz,
                             s.zz - wz * qz, s.tr, n - 1, t);
}

}  // namespace plane_cert
