// octl_forest_remove_poses (store.hip): where the rows of the point store go when poses leave it.
// __host__ __device__, so that the stand-alone host program tests/host/retire_host.cpp runs the very row map of the
// kernel over heap arrays of exactly their size (AddressSanitizer / UBSan; tests/test_cpu_retire_host.py).
//
// The store is pose-major: pose p owns the old rows [end[p - 1], end[p]) (end[-1] = 0; an empty pose repeats the
// offset of the pose in front of it, as in k_transform_poses).  shift[p], p = 0 .. P, is the number of rows of removed
// poses in front of pose p (shift[P]: all of them), so
//   - a pose is removed exactly when it is not empty and shift[p + 1] - shift[p] is its size (an empty pose has no
//     row to ask about);
//   - a row of a pose that stays moves DOWN by shift[p]:  new = old - shift[p];
//   - the new end offset of any pose is end[p] - shift[p + 1]: a removed pose reads as an empty one in the new
//     numbering, and "first pose whose new end lies behind the row" skips it like any empty pose.
// The kernel is driven by the DESTINATION (k_retire_poses writes whole 16-byte units of the new store), so it needs
// the inverse, new row -> old row, which the same two arrays give.
//
// What one call does to a built forest, in stream order (store.hip: octl_forest_remove_poses has the code):
//   1. k_retire_mask     one wave per (leaf, pose) block: the mask bytes of a removed pose's block become 0; where no
//                        RANSAC mask is pending the bytes of every other block become 1 (no fill launch).  A PENDING
//                        RANSAC mask stays in the mask and is applied by the same ONE compaction, as with
//                        octl_forest_carve and octl_forest_filter_count.
//   2. apply_device_mask the compaction of mask.hip; it clears alive flags by OLD store index, so it runs before ...
//   3. k_retire_blocks   one wave per block of the COMPACTED table: ord_idx -= shift[slot], blk_slot = new_slot[slot]
//   4. k_retire_poses    the store pass, out of place: rows and alive flags of the poses that stay, the voxel box of
//                        the alive ones among them folded into a fresh box.
// A forest without tables (never built, or reset by octl_forest_transform_poses) takes step 4 alone, and
// k_alive_count behind it: no compaction has counted the rows that left, so the flags just written are counted.
// Launches and host waits, whatever the number of points (the compaction in its fused form, mask.hip): built forest
// 4 launches, 2 host waits (the compaction's counts; the counters of this call); forest without tables 2 launches
// (1 where the flags were never written: every row alive), 1 host wait.  No pose left: the store pass is not launched;
// no block left: neither is k_retire_blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RETIRE_HD __host__ __device__ __forceinline__

struct RetireMap {
  const int64_t* end;    // [P]     OLD end offset of every pose
  const int64_t* shift;  // [P + 1] rows of removed poses in front of pose p
  int n_poses;
};

RETIRE_HD int64_t retire_new_end(const RetireMap& m, int p) { return m.end[p] - m.shift[p + 1]; }

// first pose in [lo, hi] whose OLD end lies behind old_row (old_row < end[hi]: there is one)
RETIRE_HD int retire_pose_of_old(const RetireMap& m, int lo, int hi, int64_t old_row) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (m.end[mid] > old_row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// first pose in [lo, hi] whose NEW end lies behind new_row (new_row < retire_new_end(hi): there is one); never a
// removed pose and never an empty one
RETIRE_HD int retire_pose_of_new(const RetireMap& m, int lo, int hi, int64_t new_row) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (retire_new_end(m, mid) > new_row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// old row -> new row, -1: the row's pose is removed.  0 <= old_row < end[P - 1]
RETIRE_HD int64_t retire_new_row(const RetireMap& m, int64_t old_row) {
  const int p = retire_pose_of_old(m, 0, m.n_poses - 1, old_row);
  return m.shift[p + 1] != m.shift[p] ? (int64_t)-1 : old_row - m.shift[p];
}

// new row -> old row.  0 <= new_row < end[P - 1] - shift[P]
RETIRE_HD int64_t retire_old_row(const RetireMap& m, int64_t new_row) {
  return new_row + m.shift[retire_pose_of_new(m, 0, m.n_poses - 1, new_row)];
}

// The flat form the kernel copies by: double d of the new store (row d / 3, axis d % 3) is double
// d + 3 * shift[pose of row d / 3] of the old one; [lo, hi] brackets the pose (a workgroup finds the poses of its first
// and last row once).  An odd shift puts the source 8 bytes off the destination's 16-byte units (24 mod 16 = 8).
RETIRE_HD int64_t retire_src_double(const RetireMap& m, int lo, int hi, int64_t d) {
  const int p = lo == hi ? lo : retire_pose_of_new(m, lo, hi, d / 3);
  return d + 3 * m.shift[p];
}
