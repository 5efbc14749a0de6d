// What the matching kernels of the two nearest-point registrations share (register_points.hip: k_reg_match;
// register_nearest_plane.hip: k_regn_match): the k = 1 sink of nearest_walk.  (The transform of a query: reg_fold.h.)
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
