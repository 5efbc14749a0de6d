// What the matching kernels of the two nearest-point registrations share (register_points.hip: k_reg_match;
// register_nearest_plane.hip: k_regn_match): the transform of a query and the k = 1 sink of nearest_walk.
#pragma once
#include "nearest_walk.h"

// the best candidate of a walk with k = 1, and where it lies in the ordered arrays
struct RegBest {
  double bd;
  uint64_t bid;
  uint32_t pos;
  __device__ __forceinline__ double worst() const { return bd; }
  __device__ __forceinline__ void offer(double d2, uint64_t id, uint32_t at) {
    if (cand_less(d2, id, bd, bid)) {
      bd = d2;
      bid = id;
      pos = at;
    }
  }
};

__device__ __forceinline__ void reg_transform(const double* __restrict__ T, double qx, double qy, double qz,
                                              double p[3]) {
  // (separate products and sums: the library is built with -ffp-contract=off, and the host forms the same bits)
  p[0] = ((T[0] * qx + T[1] * qy) + T[2] * qz) + T[3];
  p[1] = ((T[4] * qx + T[5] * qy) + T[6] * qz) + T[7];
  p[2] = ((T[8] * qx + T[9] * qy) + T[10] * qz) + T[11];
}
