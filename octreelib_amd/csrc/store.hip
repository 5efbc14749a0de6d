// The point store of a forest: the ingest kernels that copy (or widen, or move by a transform) a pose into it, mark its
// points alive and fold their voxel box, the kernel that moves the stored rows of poses by a rigid transform each, and
// the C entries that add, extend or move poses.
#include "forest.h"
#include "ingest_xf.h"
#include "ref_arith.h"
#include "store_retire.h"

namespace {

// ---- ingest: Grid.insert_points' storage step -------------------------------------------------------
// One pass over the new points of a pose: copies them into the forest's store (device sources),
// marks them alive and folds their top-level voxel indices - floor((p - corner) / L), grid.py:72-76 -
// into the forest's voxel bounding box, so that the build can form compact linear voxel keys without
// a pass of its own.
// The cloud is read as a FLAT array of doubles, 16 bytes per lane and instruction (a lane reading its
// own 48-byte pair of points touches every cache line three times): the bounding box needs the minimum
// and maximum per AXIS, and the axis of flat element i is i mod 3, whichever point it belongs to.
constexpr int ING_UNITS = 12;  // 16-byte units per thread

// The voxel box of one thread's values, folded per axis (k_ingest, k_ingest_f32): floor((p - corner) / L) with the
// corner at 0 (grid.py:72-76); a NaN, an infinity or a voxel index outside the window sets the domain flag instead.
struct VoxFold {
  int mn[3], mx[3];
  bool bad;
  __device__ __forceinline__ VoxFold() : bad(false) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = 1 << 30;
      mx[a] = -(1 << 30);
    }
  }
  __device__ __forceinline__ void add(double v, int axis, double L) {
    const double f = L == 1.0 ? floor(v) : floor_div_exact(v, L);  // (floor_div_exact(v, 1) == floor(v))
    if (fabs(f) < (double)OCTL_VOX_ABS_LIMIT) {  // false for NaN / inf
      const int q = (int)f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (a == axis) {
          mn[a] = min(mn[a], q);
          mx[a] = max(mx[a], q);
        }
      }
    } else {
      bad = true;
    }
  }
  // mode 1 (one cube): no fold, a box of [0, 0] from every thread that had points
  __device__ __forceinline__ void zero() { mn[0] = mn[1] = mn[2] = mx[0] = mx[1] = mx[2] = 0; }
};

// wave + block reduction of the threads' boxes (a 256-thread block, every thread calls it), then at most six atomics
// per block and only when the block widens the box (same-address atomics serialise); bbox[6] is the domain flag
__device__ __forceinline__ void vox_fold_publish(VoxFold& b, int32_t* __restrict__ bbox) {
  const int big = 1 << 30;
  __shared__ int s_bb[4][6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      b.mn[a] = min(b.mn[a], __shfl_xor(b.mn[a], off));
      b.mx[a] = max(b.mx[a], __shfl_xor(b.mx[a], off));
    }
  }
  if (__any(b.bad) && (threadIdx.x & 63) == 0) atomicExch(reinterpret_cast<uint32_t*>(bbox + 6), 1u);
  if ((threadIdx.x & 63) == 0) {
    int* w = s_bb[threadIdx.x >> 6];
    w[0] = b.mn[0]; w[1] = b.mn[1]; w[2] = b.mn[2]; w[3] = b.mx[0]; w[4] = b.mx[1]; w[5] = b.mx[2];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    int v = s_bb[0][a];
    for (int w = 1; w < 4; ++w) v = (a < 3) ? min(v, s_bb[w][a]) : max(v, s_bb[w][a]);
    if (a < 3) {
      if (v != big && v < __hip_atomic_load(&bbox[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&bbox[a], v);
    } else {
      if (v != -big && v > __hip_atomic_load(&bbox[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&bbox[a], v);
    }
  }
}

// alive flags of the new points: 16 per thread, 4096 per block (nullptr: the caller sets them otherwise)
__device__ __forceinline__ void ingest_alive(uint8_t* __restrict__ alive, int64_t n) {
  if (!alive) return;
  const int64_t a0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (a0 + 16 <= n && (reinterpret_cast<uintptr_t>(alive) & 15) == 0) {
    *reinterpret_cast<uint4*>(alive + a0) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
  } else {
    for (int64_t i = a0; i < n && i < a0 + 16; ++i) alive[i] = 1;
  }
}

template <bool COPY>
__global__ __launch_bounds__(256) void k_ingest(const double* __restrict__ src, double* __restrict__ dst,
                                                uint8_t* __restrict__ alive, int64_t n, int mode,
                                                double L, int32_t* __restrict__ bbox) {
  VoxFold box;
  const int64_t n_flat = 3 * n, n_units = n_flat / 2;
  const int64_t u0 = (int64_t)blockIdx.x * (256 * ING_UNITS) + threadIdx.x;
  // (a pose behind an odd number of stored points starts 8 bytes off: scalar accesses then)
  const bool al16 = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  double2 v[ING_UNITS];
#pragma unroll
  for (int k = 0; k < ING_UNITS; ++k) {
    const int64_t u = u0 + k * 256;
    if (u < n_units) {
      if (al16) {
        v[k] = reinterpret_cast<const double2*>(src)[u];
      } else {
        v[k].x = src[2 * u];
        v[k].y = src[2 * u + 1];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ING_UNITS; ++k) {
    const int64_t u = u0 + k * 256;
    if (u < n_units) {
      if (COPY) {
        if (al16) {
          reinterpret_cast<double2*>(dst)[u] = v[k];
        } else {
          dst[2 * u] = v[k].x;
          dst[2 * u + 1] = v[k].y;
        }
      }
      if (mode == 0) {
        const int ax = (int)((2 * u) % 3);
        box.add(v[k].x, ax, L);
        box.add(v[k].y, ax == 2 ? 0 : ax + 1, L);
      }
    }
  }
  if ((n_flat & 1) && u0 == 0) {  // the last double of an odd number of points
    const double t = src[n_flat - 1];
    if (COPY) dst[n_flat - 1] = t;
    if (mode == 0) box.add(t, 2, L);
  }
  if (mode != 0 && u0 < n_units) box.zero();
  ingest_alive(alive, n);
  vox_fold_publish(box, bbox);
}

// ---- ingest of a float32 cloud -----------------------------------------------------------------------
// The same pass for a cloud that arrives as float32 (half the PCIe bytes of f64): every value is widened with
// (double)v - exact, subnormals included - into the forest's f64 store, and the box is folded from the WIDENED value,
// so the store, the box and the domain flag are those of the cloud's f64 twin.  The flat array is read 16 bytes
// (four floats) per lane; the axis of flat element i is again i mod 3, and 4u mod 3 == u mod 3.  Each unit lands as
// two 16-byte stores where the destination is 16-byte aligned (a pose behind an even number of stored points).
constexpr int ING32_UNITS = 6;  // 16-byte float4 units per thread: 6144 floats = 2048 points per block, as k_ingest
__global__ __launch_bounds__(256) void k_ingest_f32(const float* __restrict__ src, double* __restrict__ dst,
                                                    uint8_t* __restrict__ alive, int64_t n, int mode,
                                                    double L, int32_t* __restrict__ bbox) {
  VoxFold box;
  const int64_t n_flat = 3 * n, n_units = n_flat / 4;
  const int64_t u0 = (int64_t)blockIdx.x * (256 * ING32_UNITS) + threadIdx.x;
  // (a view that starts at row 1 of a float32 array is only 4-byte aligned; an odd store offset puts dst 8 bytes off)
  const bool src16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const bool dst16 = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  float4 v[ING32_UNITS];
#pragma unroll
  for (int k = 0; k < ING32_UNITS; ++k) {
    const int64_t u = u0 + k * 256;
    if (u < n_units) {
      if (src16) {
        v[k] = reinterpret_cast<const float4*>(src)[u];
      } else {
        v[k].x = src[4 * u];
        v[k].y = src[4 * u + 1];
        v[k].z = src[4 * u + 2];
        v[k].w = src[4 * u + 3];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ING32_UNITS; ++k) {
    const int64_t u = u0 + k * 256;
    if (u < n_units) {
      const double2 lo = make_double2((double)v[k].x, (double)v[k].y);
      const double2 hi = make_double2((double)v[k].z, (double)v[k].w);
      if (dst16) {
        reinterpret_cast<double2*>(dst)[2 * u] = lo;
        reinterpret_cast<double2*>(dst)[2 * u + 1] = hi;
      } else {
        dst[4 * u] = lo.x;
        dst[4 * u + 1] = lo.y;
        dst[4 * u + 2] = hi.x;
        dst[4 * u + 3] = hi.y;
      }
      if (mode == 0) {
        const int ax = (int)(u % 3);
        box.add(lo.x, ax, L);
        box.add(lo.y, ax == 2 ? 0 : ax + 1, L);
        box.add(hi.x, ax == 0 ? 2 : ax - 1, L);
        box.add(hi.y, ax, L);
      }
    }
  }
  // the last 1-3 floats when 3n is not a multiple of 4 (n < 2 has no full unit at all)
  const int64_t rest = 4 * n_units;
  if (rest < n_flat && u0 == 0) {
    for (int64_t i = rest; i < n_flat; ++i) {
      const double t = (double)src[i];
      dst[i] = t;
      if (mode == 0) box.add(t, (int)(i % 3), L);
    }
  }
  if (mode != 0 && (u0 < n_units || (u0 == 0 && n_flat > 0))) box.zero();
  ingest_alive(alive, n);
  vox_fold_publish(box, bbox);
}

// ---- ingest under a transform ------------------------------------------------------------------------------------
// The same pass for a cloud that is inserted under one 3x4 (SEG = false: the matrix is a kernel argument, uniform) or
// under a table of up to OCTL_XF_MAX_SEGMENTS of them with one uint16 index per row (SEG = true: "piecewise rigid").
// The store, the alive flags and the box folded from the MOVED values are those of the cloud's host-transformed twin
// (registration.py: transform_rows_np).  A lane needs the three coordinates of a row, so the cloud is read in row
// groups (ingest_xf.h has the thread's body, which the host test compiles too); src == dst for an f64 host cloud, which
// is uploaded into the store and moved in place (hence no __restrict__ on the two).  The table stays in global memory:
// 96 KB at most, L2-resident, read through scalar loads where a wave agrees on its index (sweep order) and gathered per
// lane elsewhere; no LDS copy (a workgroup of 1024 rows would stage up to 96 KB to use a few rows of it).
struct IxfFold {
  VoxFold box;
  int mode;
  double L;
  bool any = false;
  __device__ __forceinline__ void row(double x, double y, double z) {
    any = true;
    if (mode == 0) {
      box.add(x, 0, L);
      box.add(y, 1, L);
      box.add(z, 2, L);
    }
  }
};

template <bool F32, bool SEG, bool SRC16, bool DST16>
__global__ __launch_bounds__(256) void k_ingest_xf(const void* src, double* dst, uint8_t* __restrict__ alive, int64_t n,
                                                   const IxfMat one, const IxfMat* __restrict__ table, int n_tab,
                                                   const uint16_t* __restrict__ seg, int mode, double L,
                                                   int32_t* __restrict__ bbox) {
  IxfFold fold;
  fold.mode = mode;
  fold.L = L;
  const int64_t g0 = (int64_t)blockIdx.x * (256 * IXF_GROUPS) + threadIdx.x;
  ingest_xf_thread<F32, SEG, SRC16, DST16>(src, dst, seg, one, table, n_tab, n, g0, fold);
  if (mode != 0 && fold.any) fold.box.zero();
  ingest_alive(alive, n);
  vox_fold_publish(fold.box, bbox);
}

// ---- transform_poses: the stored rows of the selected poses moved by one rigid transform each --------------------
// One pass over the WHOLE store, out of place: a row of a selected pose becomes ((R_i0 x + R_i1 y) + R_i2 z) + t_i
// (registration.py: transform_np - every product and sum rounded, the library is built without contraction), a row of
// any other pose is copied bit for bit (1 * -0.0 + 0 * y would lose the sign), and the alive rows are folded into a
// FRESH voxel box, which is where a moved coordinate outside the domain shows.  Dead rows travel along (their
// coordinates mean nothing) and stay out of the box and of the domain flag.
// A thread owns XF_PAIRS pairs of consecutive rows (2p, 2p + 1): 48 bytes = three 16-byte units, and a pair starts
// 16-byte aligned whatever the poses' sizes because the store starts aligned.  A pose may start at an odd row, so the
// two rows of one pair - and the rows of one workgroup - can belong to different poses: the pose of a row is found
// from the end offsets (ascending; an empty pose has the end of the one before it).
constexpr int XF_PAIRS = 2;                        // row pairs per thread
constexpr int XF_ROWS_PER_WG = 256 * 2 * XF_PAIRS; // 1024

// the table one call uploads: the box the kernel folds into, the end offset of every pose, then per pose the 3x4 and
// whether the pose is selected
struct XfSlot {
  double m[12];
  int64_t selected;
  int64_t pad;  // (112 bytes: every record starts 16-byte aligned)
};
struct XfLayout {
  Carve plan;
  Carve::Part<int32_t> box = plan.add<int32_t>(8);
  Carve::Part<int64_t> end;
  Carve::Part<XfSlot> slot;
  explicit XfLayout(int n_poses) : end(plan.add<int64_t>((size_t)n_poses)), slot(plan.add<XfSlot>((size_t)n_poses)) {}
};

// first pose at or behind `s` whose end offset lies behind `row` (row < n_store = end[n_poses - 1]: there is one)
__device__ __forceinline__ int xf_pose_of(const int64_t* __restrict__ end, int s, int n_poses, int64_t row) {
  int lo = s, hi = n_poses - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (end[mid] > row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_transform_poses(const double* __restrict__ src, double* __restrict__ dst,
                                                         const uint8_t* __restrict__ alive /* nullptr: all alive */,
                                                         int64_t n, const int64_t* __restrict__ end,
                                                         const XfSlot* __restrict__ slots, int n_poses, int mode,
                                                         double L, double c0, double c1, double c2,
                                                         int32_t* __restrict__ bbox) {
  VoxFold box;
  const int64_t p0 = (int64_t)blockIdx.x * (256 * XF_PAIRS) + threadIdx.x;
  const bool al16 = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  double2 v[XF_PAIRS][3];
  uint32_t live[XF_PAIRS];
#pragma unroll
  for (int k = 0; k < XF_PAIRS; ++k) {
    const int64_t r = 2 * (p0 + k * 256);
    live[k] = 0;
    v[k][0] = v[k][1] = v[k][2] = make_double2(0.0, 0.0);
    if (r + 1 < n) {
      if (al16) {
        const double2* s2 = reinterpret_cast<const double2*>(src) + 3 * (p0 + k * 256);
        v[k][0] = s2[0];
        v[k][1] = s2[1];
        v[k][2] = s2[2];
      } else {
        const double* s1 = src + 3 * r;
        v[k][0] = make_double2(s1[0], s1[1]);
        v[k][1] = make_double2(s1[2], s1[3]);
        v[k][2] = make_double2(s1[4], s1[5]);
      }
      // (the flags' block is 16-byte aligned and r is even)
      live[k] = alive ? (uint32_t)*reinterpret_cast<const uint16_t*>(alive + r) : 0x0101u;
    } else if (r < n) {  // the last row of an odd number of rows
      const double* s1 = src + 3 * r;
      v[k][0] = make_double2(s1[0], s1[1]);
      v[k][1].x = s1[2];
      live[k] = alive ? (uint32_t)alive[r] : 1u;
    }
  }
  // the poses of the thread's first and last row bracket those of every row between them
  const int64_t r_first = 2 * p0, r_last = min(2 * (p0 + (XF_PAIRS - 1) * 256) + 1, n - 1);
  int s_lo = 0, s_hi = 0;
  if (r_first < n) {
    s_lo = xf_pose_of(end, 0, n_poses, r_first);
    s_hi = end[s_lo] > r_last ? s_lo : xf_pose_of(end, s_lo, n_poses, r_last);
  }
  int cur = -1;
  bool sel = false, any_alive = false;
  double m[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) m[j] = 0.0;
#pragma unroll
  for (int k = 0; k < XF_PAIRS; ++k) {
    const int64_t r = 2 * (p0 + k * 256);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (r + h >= n) continue;
      const int s = s_lo == s_hi ? s_lo : xf_pose_of(end, s_lo, n_poses, r + h);
      if (s != cur) {
        cur = s;
        sel = slots[s].selected != 0;
        if (sel) {
#pragma unroll
          for (int j = 0; j < 12; ++j) m[j] = slots[s].m[j];
        }
      }
      double x = h ? v[k][1].y : v[k][0].x, y = h ? v[k][2].x : v[k][0].y, z = h ? v[k][2].y : v[k][1].x;
      if (sel) {
        const double tx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        const double ty = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        const double tz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
        x = tx, y = ty, z = tz;
        if (h) {
          v[k][1].y = x, v[k][2].x = y, v[k][2].y = z;
        } else {
          v[k][0].x = x, v[k][0].y = y, v[k][1].x = z;
        }
      }
      if ((live[k] >> (8 * h)) & 0xFFu) {
        any_alive = true;
        if (mode == 0) {
          box.add(x, 0, L);
          box.add(y, 1, L);
          box.add(z, 2, L);
        } else {
          // the root's placement test (octree.py:73-75,94-98): 0 <= fl(p - c) < e on every axis, NaN fails
          const double dx = x - c0, dy = y - c1, dz = z - c2;
          if (!(dx >= 0.0 && dx < L && dy >= 0.0 && dy < L && dz >= 0.0 && dz < L)) box.bad = true;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < XF_PAIRS; ++k) {
    const int64_t r = 2 * (p0 + k * 256);
    if (r + 1 < n) {
      if (al16) {
        double2* d2 = reinterpret_cast<double2*>(dst) + 3 * (p0 + k * 256);
        d2[0] = v[k][0];
        d2[1] = v[k][1];
        d2[2] = v[k][2];
      } else {
        double* d1 = dst + 3 * r;
        d1[0] = v[k][0].x, d1[1] = v[k][0].y, d1[2] = v[k][1].x;
        d1[3] = v[k][1].y, d1[4] = v[k][2].x, d1[5] = v[k][2].y;
      }
    } else if (r < n) {
      double* d1 = dst + 3 * r;
      d1[0] = v[k][0].x, d1[1] = v[k][0].y, d1[2] = v[k][1].x;
    }
  }
  if (mode != 0 && any_alive) box.zero();
  vox_fold_publish(box, bbox);
}

// ---- remove_poses: the store squeezed, the rows of the removed poses gone (store_retire.h) --------
// One pass over the NEW store, out of place: later poses move DOWN past the removed ones, so a copy in place would
// race between workgroups.  The copy is flat, like k_ingest's: a lane owns whole 16-byte units of the DESTINATION
// (two doubles) and stores them with one instruction each whatever the shift.  The source of a unit lies
// 3 * shift doubles further up: 16-byte aligned too when the shift is even (one 16-byte load); 8 bytes off when it is
// odd - a removed pose with an odd number of rows in front, 24 mod 16 = 8 - and then the two doubles are loaded one
// by one (the store stays wide).  The unit where two poses of different shifts meet takes each double by its own.
// All twelve row loads of a thread are issued first.  Behind them the alive flags of the workgroup's 2048 rows are
// gathered (8 per thread, one 8-byte store) and kept in LDS; behind a barrier they tell the fold which of the loaded
// doubles count: VoxFold / vox_fold_publish over the alive rows that stay, into a fresh box.
// (No counter of the alive rows in this kernel: one same-address atomicAdd per workgroup - 3 256 of them for 6.7 M
// rows - took it from 96 to 166 us; a forest without tables counts the new flags in k_alive_count.)
constexpr int RT_UNITS = 12;                                // 16-byte units per thread
constexpr int RT_ROWS_PER_WG = 256 * RT_UNITS * 2 / 3;      // 2048

// the table one call uploads: the fresh box with the call's two counters {rows of removed poses the compaction took
// out, alive rows that stay} behind it, the poses' old end offsets, their shifts, new slots and the selection
struct RetireLayout {
  Carve plan;
  Carve::Part<int32_t> box = plan.add<int32_t>(12);  // (words 8..11: the two u64 counters)
  Carve::Part<int64_t> end, shift;
  Carve::Part<int32_t> new_slot;
  Carve::Part<uint8_t> sel;
  explicit RetireLayout(int n_poses)
      : end(plan.add<int64_t>((size_t)n_poses)), shift(plan.add<int64_t>((size_t)n_poses + 1)),
        new_slot(plan.add<int32_t>((size_t)n_poses)), sel(plan.add<uint8_t>((size_t)n_poses)) {}
};

__global__ __launch_bounds__(256) void k_retire_poses(const double* __restrict__ src, double* __restrict__ dst,
                                                      const uint8_t* __restrict__ alive /* nullptr: all alive */,
                                                      uint8_t* __restrict__ alive_out, int64_t n_new,
                                                      const int64_t* __restrict__ end,
                                                      const int64_t* __restrict__ shift, int n_poses, int mode,
                                                      double L, int32_t* __restrict__ bbox) {
  __shared__ __align__(8) uint8_t s_alive[RT_ROWS_PER_WG];
  const RetireMap m{end, shift, n_poses};
  const int t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * RT_ROWS_PER_WG;  // (< n_new: the grid is ceil(n_new / 2048))
  // the poses of the workgroup's first and last row bracket those of every row between them; as a rule they are one
  // pose, and the whole workgroup moves by one shift
  const int64_t r_last = min(row0 + RT_ROWS_PER_WG, n_new) - 1;
  const int s_lo = retire_pose_of_new(m, 0, n_poses - 1, row0);
  const int s_hi = retire_new_end(m, s_lo) > r_last ? s_lo : retire_pose_of_new(m, s_lo, n_poses - 1, r_last);
  const bool one = s_lo == s_hi;
  const int64_t sh = shift[s_lo];
  // ---- the rows: units u0 + 256 k of the new store, doubles 2 u and 2 u + 1; every load is issued before the flags
  const int64_t n_flat = 3 * n_new, n_units = n_flat / 2;
  const int64_t u0 = (int64_t)blockIdx.x * (256 * RT_UNITS) + t;   // (row0 * 3 / 2 = blockIdx * 3072)
  double2 v[RT_UNITS];
#pragma unroll
  for (int k = 0; k < RT_UNITS; ++k) {
    const int64_t u = u0 + k * 256;
    v[k] = make_double2(0.0, 0.0);
    if (u < n_units) {
      if (one && (sh & 1) == 0) {
        v[k] = *reinterpret_cast<const double2*>(src + 2 * u + 3 * sh);   // (the store starts 16-byte aligned)
      } else if (one) {
        v[k].x = src[2 * u + 3 * sh];
        v[k].y = src[2 * u + 3 * sh + 1];
      } else {
        const int64_t a = retire_src_double(m, s_lo, s_hi, 2 * u), b = retire_src_double(m, s_lo, s_hi, 2 * u + 1);
        if (b == a + 1 && (a & 1) == 0) {
          v[k] = *reinterpret_cast<const double2*>(src + a);
        } else {
          v[k].x = src[a];
          v[k].y = src[b];
        }
      }
    }
  }
  // ---- alive flags: rows row0 + 8 t .. + 7, normalised to 0 / 1
  {
    const int64_t r = row0 + 8 * t;
    uint64_t w = 0;
    if (!alive) {
      for (int j = 0; j < 8 && r + j < n_new; ++j) w |= (uint64_t)1 << (8 * j);
    } else if (one && r + 8 <= n_new && ((r + sh) & ~(int64_t)7) + 16 <= n_new + shift[n_poses]) {
      // one shift: the eight flags from the two aligned 8-byte words that hold them (both inside the old flags)
      const int64_t q = (r + sh) & ~(int64_t)7;
      const int o = (int)((r + sh) & 7);
      const uint64_t lo = *reinterpret_cast<const uint64_t*>(alive + q);
      const uint64_t hi = *reinterpret_cast<const uint64_t*>(alive + q + 8);
      const uint64_t x = o ? (lo >> (8 * o)) | (hi << (64 - 8 * o)) : lo;
      w = ((((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) >> 7) & 0x0101010101010101ull;
    } else {
      for (int j = 0; j < 8 && r + j < n_new; ++j) {
        const int p = one ? s_lo : retire_pose_of_new(m, s_lo, s_hi, r + j);
        w |= (uint64_t)(alive[r + j + shift[p]] ? 1 : 0) << (8 * j);
      }
    }
    *reinterpret_cast<uint64_t*>(s_alive + 8 * t) = w;
    if (alive_out) {
      if (r + 8 <= n_new) {
        *reinterpret_cast<uint64_t*>(alive_out + r) = w;   // (the flags' block is 16-byte aligned, r a multiple of 8)
      } else {
        for (int j = 0; j < 8 && r + j < n_new; ++j) alive_out[r + j] = (uint8_t)(w >> (8 * j));
      }
    }
  }
  __syncthreads();
  VoxFold box;
  bool any_alive = false;
#pragma unroll
  for (int k = 0; k < RT_UNITS; ++k) {
    const int64_t u = u0 + k * 256;
    if (u < n_units) {
      reinterpret_cast<double2*>(dst)[u] = v[k];
      const int ld = 2 * (t + k * 256);                      // double within the workgroup: row ld / 3, axis ld % 3
      const int r0 = ld / 3, a0 = ld - 3 * r0, r1 = (ld + 1) / 3, a1 = ld + 1 - 3 * r1;
      const bool l0 = s_alive[r0] != 0, l1 = s_alive[r1] != 0;
      any_alive |= l0 | l1;
      if (mode == 0) {
        if (l0) box.add(v[k].x, a0, L);
        if (l1) box.add(v[k].y, a1, L);
      }
    }
  }
  if ((n_flat & 1) && u0 == 0) {  // the last double of an odd number of rows: the z of row n_new - 1
    const int p = retire_pose_of_new(m, 0, n_poses - 1, n_new - 1);
    const double z = src[n_flat - 1 + 3 * shift[p]];
    dst[n_flat - 1] = z;
    const bool l = alive ? alive[n_new - 1 + shift[p]] != 0 : true;
    any_alive |= l;
    if (mode == 0 && l) box.add(z, 2, L);
  }
  if (mode != 0 && any_alive) box.zero();
  vox_fold_publish(box, bbox);
}

// the alive rows of a squeezed store that has no block table to say so (a forest without tables): flags are 0 / 1, 16
// per lane and step, one atomic per workgroup of a grid that does not grow with the store
__global__ __launch_bounds__(256) void k_alive_count(const uint8_t* __restrict__ alive, int64_t n,
                                                     unsigned long long* __restrict__ out) {
  __shared__ uint32_t s_w[4];
  uint32_t c = 0;
  const int64_t n16 = n / 16;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
    const uint4 w = reinterpret_cast<const uint4*>(alive)[i];
    c += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < n - 16 * n16) c += alive[16 * n16 + threadIdx.x];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0 && s_w[0] + s_w[1] + s_w[2] + s_w[3])
    atomicAdd(out, (unsigned long long)(s_w[0] + s_w[1] + s_w[2] + s_w[3]));
}

// the blocks that stay, in the COMPACTED block table: their points are named by their new store rows, their pose by
// its new slot.  One wavefront per block; lane 0 alone touches the block's slot word.
__global__ __launch_bounds__(256) void k_retire_blocks(const uint32_t* __restrict__ blk_start,
                                                       const int32_t* __restrict__ blk_size,
                                                       int32_t* __restrict__ blk_slot, int64_t nb,
                                                       const int64_t* __restrict__ shift,
                                                       const int32_t* __restrict__ new_slot,
                                                       uint32_t* __restrict__ ord_idx) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  const int lane = threadIdx.x & 63;
  int s = 0;
  if (lane == 0) {
    s = blk_slot[b];
    blk_slot[b] = new_slot[s];
  }
  s = __shfl(s, 0);
  const uint32_t sh = (uint32_t)shift[s];
  const int64_t n = blk_size[b], s0 = blk_start[b];
  if (sh)
    for (int64_t i = lane; i < n; i += 64) ord_idx[s0 + i] -= sh;
}

__global__ void k_bbox_reset(int32_t* __restrict__ bbox) {
  const int a = threadIdx.x;
  if (a < 8) bbox[a] = a < 3 ? (1 << 30) : (a < 6 ? -(1 << 30) : 0);
}

// Device sources are consumed in stream order (no synchronisation: the caller keeps the buffer
// unchanged until the next synchronising call on the context); host sources are copied before the
// call returns.
// What every append does before its launches: the store, the alive flags and the box are ready for n more points, and
// *dst / *alive point at the new points' place in the store and in the alive flags.
int store_prepare_append(octl_forest* f, const void* xyz, int64_t n, double** dst, uint8_t** alive) {
  octl_ctx* ctx = f->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n < 0 || (n > 0 && !xyz)) return octl_set_error(ctx, OCTL_E_INVALID, "bad point buffer");
  const int64_t total = f->n_store + n;
  if (total >= ((int64_t)1 << 31))
    return octl_set_error(ctx, OCTL_E_INVALID, "more than 2^31-1 points in one forest");
  // a store that is read in place from the caller's buffer becomes the forest's own before it grows; a
  // cloud whose box has not been taken yet is folded in now (the kernel below only adds the new points)
  if (f->store_borrowed) OCTL_TRY(store_materialize(f));
  if (f->bbox_pending) OCTL_TRY(store_compute_bbox(f));
  OCTL_TRY(alive_ensure(f));   // (the flags of the points in front of the new ones: the buffer may move)
  OCTL_TRY(devbuf_reserve(ctx, f->xyz, (size_t)std::max<int64_t>(total, 1) * 24 + 16, 1));
  OCTL_TRY(devbuf_reserve(ctx, f->alive, (size_t)std::max<int64_t>(total, 1) + 2, 1));
  OCTL_TRY(bbox_ensure(f));
  *dst = f->xyz.as<double>() + 3 * f->n_store;
  *alive = f->alive.as<uint8_t>() + f->n_store;
  return OCTL_OK;
}

// ... and behind its launches (the box stays on the device: the build forms the key geometry there, or fetches it
// when it has to)
int store_append_done(octl_ctx* ctx, bool from_device) {
  HIP_TRY(ctx, hipGetLastError());
  if (!from_device) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the host buffer is the caller's again
  return OCTL_OK;
}

int store_append(octl_forest* f, const double* xyz, int64_t n, bool from_device) {
  octl_ctx* ctx = f->ctx;
  double* dst = nullptr;
  uint8_t* alive = nullptr;
  OCTL_TRY(store_prepare_append(f, xyz, n, &dst, &alive));
  if (n > 0) {
    hipStream_t st = ctx->stream;
    const unsigned grid = (unsigned)std::max<int64_t>(1, ceil_div(3 * n / 2, 256 * ING_UNITS));
    KTimer t(ctx, "ingest");
    // (an odd store offset would misalign the 16-byte accesses of the pair-wise kernel: such a pose
    //  goes through the plain copy + the in-place form on its own, 8-byte aligned, pointer)
    const bool aligned = (f->n_store % 2) == 0 && (reinterpret_cast<uintptr_t>(xyz) % 16) == 0;
    if (from_device && xyz == dst) {
      // an adopted buffer (store_adopt): the points are in place already
      OCTL_LAUNCH(k_ingest<false>, dim3(grid), dim3(256), 0, st, (const double*)dst, dst, alive, n,
                         f->mode, f->edge, f->bbox_dev.as<int32_t>());
    } else if (from_device && aligned) {
      OCTL_LAUNCH(k_ingest<true>, dim3(grid), dim3(256), 0, st, xyz, dst, alive, n, f->mode,
                         f->edge, f->bbox_dev.as<int32_t>());
    } else {
      HIP_TRY(ctx, hipMemcpyAsync(dst, xyz, (size_t)n * 24,
                                  from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
      if ((f->n_store % 2) == 0) {
        OCTL_LAUNCH(k_ingest<false>, dim3(grid), dim3(256), 0, st, (const double*)dst, dst, alive,
                           n, f->mode, f->edge, f->bbox_dev.as<int32_t>());
      } else {
        // first point alone, then the aligned rest
        OCTL_LAUNCH(k_ingest<false>, dim3(1), dim3(256), 0, st, (const double*)dst, dst, alive,
                           (int64_t)1, f->mode, f->edge, f->bbox_dev.as<int32_t>());
        if (n > 1)
          OCTL_LAUNCH(k_ingest<false>, dim3((unsigned)std::max<int64_t>(1, ceil_div(3 * (n - 1) / 2, 256 * ING_UNITS))), dim3(256),
                             0, st, (const double*)(dst + 3), dst + 3, alive + 1, n - 1, f->mode, f->edge,
                             f->bbox_dev.as<int32_t>());
      }
    }
    OCTL_TRY(store_append_done(ctx, from_device));
  }
  return OCTL_OK;
}

// The same for a float32 cloud: k_ingest_f32 widens it into the f64 store, so the forest holds exactly what
// store_append of the cloud's f64 twin leaves.  A device source is never read in place (everything downstream reads
// the store as f64); a host source is uploaded into the context's staging buffer first (12 B per point over PCIe).
int store_append_f32(octl_forest* f, const float* xyz, int64_t n, bool from_device) {
  octl_ctx* ctx = f->ctx;
  double* dst = nullptr;
  uint8_t* alive = nullptr;
  OCTL_TRY(store_prepare_append(f, xyz, n, &dst, &alive));
  if (n > 0) {
    hipStream_t st = ctx->stream;
    const float* src = xyz;
    if (!from_device) OCTL_TRY(devbuf_reserve(ctx, ctx->f32_stage, (size_t)n * 12 + 16));
    KTimer t(ctx, "ingest_f32");
    if (!from_device) {
      HIP_TRY(ctx, hipMemcpyAsync(ctx->f32_stage.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
      src = ctx->f32_stage.as<float>();
    }
    const unsigned grid = (unsigned)std::max<int64_t>(1, ceil_div(3 * n / 4, 256 * ING32_UNITS));
    OCTL_LAUNCH(k_ingest_f32, dim3(grid), dim3(256), 0, st, src, dst, alive, n, f->mode, f->edge,
                f->bbox_dev.as<int32_t>());
    OCTL_TRY(store_append_done(ctx, from_device));
  }
  return OCTL_OK;
}

// The arguments of a cloud under a transform (octl_forest_add_pose_xf / _extend_pose_xf), checked
struct XfArgs {
  uint32_t flags;
  const double* transforms;
  int32_t n_transforms;
  const uint16_t* segment;
  bool f32() const { return (flags & OCTL_XF_F32) != 0; }
  bool device() const { return (flags & OCTL_XF_DEVICE) != 0; }
};

int xf_args_check(octl_ctx* ctx, const XfArgs& a, const void* xyz, int64_t n) {
  const int M = a.n_transforms;
  if (M < 1 || M > OCTL_XF_MAX_SEGMENTS)
    return octl_set_error(ctx, OCTL_E_INVALID, "ingest under a transform: %d transforms (1..%d)", M, OCTL_XF_MAX_SEGMENTS);
  if (!a.transforms) return octl_set_error(ctx, OCTL_E_INVALID, "ingest under a transform: null transforms");
  if (a.flags & ~(uint32_t)(OCTL_XF_F32 | OCTL_XF_DEVICE))
    return octl_set_error(ctx, OCTL_E_INVALID, "ingest under a transform: unknown flags");
  if (M > 1 && !a.segment)
    return octl_set_error(ctx, OCTL_E_INVALID, "ingest under a transform: %d transforms without a segment array", M);
  if (n < 0 || (n > 0 && !xyz)) return octl_set_error(ctx, OCTL_E_INVALID, "bad point buffer");
  for (int k = 0; k < 12 * M; ++k)
    if (!std::isfinite(a.transforms[k]))
      return octl_set_error(ctx, OCTL_E_INVALID, "ingest under a transform: transform %d is not finite", k / 12);
  return OCTL_OK;
}

// store_append / store_append_f32 with the rows moved on their way into the store (k_ingest_xf).  One launch whatever
// n and whatever the store's parity.  An f64 host cloud is uploaded into the store itself and moved in place; an f32
// host cloud goes through the context's f32 staging buffer; a device cloud is read where it lies.  With a segment
// array the table and the indices (2 B per row) are uploaded by the same call.
int store_append_xf(octl_forest* f, const void* xyz, int64_t n, const XfArgs& a) {
  octl_ctx* ctx = f->ctx;
  double* dst = nullptr;
  uint8_t* alive = nullptr;
  OCTL_TRY(store_prepare_append(f, xyz, n, &dst, &alive));
  if (n == 0) return OCTL_OK;
  hipStream_t st = ctx->stream;
  const bool f32 = a.f32(), dev = a.device(), seg = a.segment != nullptr;
  const int M = a.n_transforms;
  IxfMat one;
  std::memcpy(one.m, a.transforms, sizeof one.m);  // (SEG: unused by the kernel)
  // table | indices, each from a 256-byte boundary
  const size_t tab_bytes = align256((size_t)M * sizeof(IxfMat)), seg_bytes = (size_t)n * 2;
  if (seg) OCTL_TRY(devbuf_reserve(ctx, ctx->xf_stage, tab_bytes + seg_bytes + 16));
  if (f32 && !dev) OCTL_TRY(devbuf_reserve(ctx, ctx->f32_stage, (size_t)n * 12 + 16));
  const char* up_tab = reinterpret_cast<const char*>(a.transforms);
  const char* up_seg = reinterpret_cast<const char*>(a.segment);
  if (seg && dev) {
    // no host wait in this call: the uploads read the library's copy of the two arrays
    if (!ctx->xf_event) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->xf_event, hipEventDisableTiming));
    if (ctx->xf_inflight && hipEventQuery(ctx->xf_event) != hipSuccess) {
      (void)hipGetLastError();                           // (hipErrorNotReady is not an error here)
      HIP_TRY(ctx, hipEventSynchronize(ctx->xf_event));  // (the previous call's upload is still reading the copy)
    }
    ctx->xf_inflight = false;
    ctx->xf_host.resize(tab_bytes + seg_bytes);
    std::memcpy(ctx->xf_host.data(), a.transforms, (size_t)M * sizeof(IxfMat));
    std::memcpy(ctx->xf_host.data() + tab_bytes, a.segment, seg_bytes);
    up_tab = ctx->xf_host.data();
    up_seg = ctx->xf_host.data() + tab_bytes;
  }
  const IxfMat* table_d = nullptr;
  const uint16_t* seg_d = nullptr;
  if (seg) {
    char* base = static_cast<char*>(ctx->xf_stage.p);
    HIP_TRY(ctx, hipMemcpyAsync(base, up_tab, (size_t)M * sizeof(IxfMat), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(base + tab_bytes, up_seg, seg_bytes, hipMemcpyHostToDevice, st));
    if (dev) {
      HIP_TRY(ctx, hipEventRecord(ctx->xf_event, st));
      ctx->xf_inflight = true;
    }
    table_d = reinterpret_cast<const IxfMat*>(base);
    seg_d = reinterpret_cast<const uint16_t*>(base + tab_bytes);
  }
  const void* src = xyz;
  if (!dev) {
    void* up = f32 ? ctx->f32_stage.p : static_cast<void*>(dst);
    HIP_TRY(ctx, hipMemcpyAsync(up, xyz, (size_t)n * (f32 ? 12 : 24), hipMemcpyHostToDevice, st));
    src = up;
  }
  const unsigned grid = (unsigned)ceil_div(n, f32 ? ixf_rows_per_wg<true>() : ixf_rows_per_wg<false>());
  int32_t* bbox = f->bbox_dev.as<int32_t>();
  // (a device cloud handed over through the ABI may be 8-byte (f64) / 4-byte (f32) aligned only; a pose behind an odd
  //  number of stored rows starts 8 bytes off: element-wise accesses on that side then, 16-byte ones on the other)
  const int src16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0, dst16 = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#define IXF_CASE(F32, SEG, S16, D16)                                                                              \
  case ((F32) << 3 | (SEG) << 2 | (S16) << 1 | (D16)):                                                            \
    OCTL_LAUNCH((k_ingest_xf<F32, SEG, S16, D16>), dim3(grid), dim3(256), 0, st, src, dst, alive, n, one, table_d, \
                M, seg_d, f->mode, f->edge, bbox);                                                                \
    break;
  {
    KTimer t(ctx, f32 ? "ingest_xf_f32" : "ingest_xf");  // (the kernel alone: the uploads are in front of it)
    switch ((int)f32 << 3 | (int)seg << 2 | src16 << 1 | dst16) {
      IXF_CASE(0, 0, 0, 0) IXF_CASE(0, 0, 0, 1) IXF_CASE(0, 0, 1, 0) IXF_CASE(0, 0, 1, 1)
      IXF_CASE(0, 1, 0, 0) IXF_CASE(0, 1, 0, 1) IXF_CASE(0, 1, 1, 0) IXF_CASE(0, 1, 1, 1)
      IXF_CASE(1, 0, 0, 0) IXF_CASE(1, 0, 0, 1) IXF_CASE(1, 0, 1, 0) IXF_CASE(1, 0, 1, 1)
      IXF_CASE(1, 1, 0, 0) IXF_CASE(1, 1, 0, 1) IXF_CASE(1, 1, 1, 0) IXF_CASE(1, 1, 1, 1)
    }
  }
#undef IXF_CASE
  return store_append_done(ctx, dev);
}

// An EMPTY forest takes the n points that f->xyz already holds (a swapped-in routed buffer, a borrowed
// caller buffer) as its first pose without touching them: alive flags by memset, the voxel box left to the
// build (bbox_pending).
int store_take_in_place(octl_forest* f, int64_t n) {
  octl_ctx* ctx = f->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (n >= ((int64_t)1 << 31))
    return octl_set_error(ctx, OCTL_E_INVALID, "more than 2^31-1 points in one forest");
  OCTL_TRY(devbuf_reserve(ctx, f->alive, (size_t)std::max<int64_t>(n, 1) + 2, 0));
  if (!f->bbox_dev.p) {
    OCTL_TRY(devbuf_reserve(ctx, f->bbox_dev, 32));
    f->bbox_stale = true;
  }
  // (no launch here: the flags are written when something needs them, the box is reset by whoever fills it)
  f->alive_stale = true;
  f->bbox_pending = true;
  return OCTL_OK;
}

}  // namespace

int bbox_ensure(octl_forest* f) {
  octl_ctx* ctx = f->ctx;
  // (no page-locked mirror per forest: hipHostMalloc / hipHostFree synchronise the whole device - also the copy
  //  stream's upload of the next scan; the one readback of the box goes through the context's scalar mirror)
  if (!f->bbox_dev.p) {
    OCTL_TRY(devbuf_reserve(ctx, f->bbox_dev, 32));
    f->bbox_stale = true;
  }
  if (!f->bbox_stale) return OCTL_OK;
  OCTL_LAUNCH(k_bbox_reset, dim3(1), dim3(64), 0, ctx->stream, f->bbox_dev.as<int32_t>());
  HIP_TRY(ctx, hipGetLastError());
  f->bbox_stale = false;
  return OCTL_OK;
}

int alive_ensure(octl_forest* f) {
  if (!f->alive_stale) return OCTL_OK;
  if (f->n_store > 0) HIP_TRY(f->ctx, hipMemsetAsync(f->alive.p, 1, (size_t)f->n_store, f->ctx->stream));
  f->alive_stale = false;
  return OCTL_OK;
}

// An empty store takes over a library-owned device buffer that holds the cloud (and hands its own
// buffer back in exchange) instead of copying it: the routed cloud of the multi-GPU path.
int store_adopt(octl_forest* f, DevBuf& src, int64_t n, bool* adopted) {
  *adopted = !(f->n_store != 0 || n <= 0 || src.cap < (size_t)n * 24 + 16 || f->store_borrowed);
  if (!*adopted) return store_append(f, src.as<double>(), n, true);
  std::swap(f->xyz, src);
  return store_take_in_place(f, n);
}

int store_compute_bbox(octl_forest* f) {
  octl_ctx* ctx = f->ctx;
  f->bbox_pending = false;
  const int64_t n = f->n_store;
  if (n <= 0) return OCTL_OK;
  OCTL_TRY(bbox_ensure(f));
  KTimer t(ctx, "ingest");
  const unsigned grid = (unsigned)std::max<int64_t>(1, ceil_div(3 * n / 2, 256 * ING_UNITS));
  double* p = f->xyz.as<double>();
  OCTL_LAUNCH(k_ingest<false>, dim3(grid), dim3(256), 0, ctx->stream, (const double*)p, p,
                     (uint8_t*)nullptr, n, f->mode, f->edge, f->bbox_dev.as<int32_t>());
  HIP_TRY(ctx, hipGetLastError());
  return OCTL_OK;
}

int store_materialize(octl_forest* f) {
  octl_ctx* ctx = f->ctx;
  if (!f->store_borrowed) return OCTL_OK;
  DevBuf own = f->xyz_own;
  f->xyz_own = DevBuf{};
  const int rc = devbuf_reserve(ctx, own, (size_t)std::max<int64_t>(f->n_store, 1) * 24 + 16, 0);
  if (rc != OCTL_OK) {
    f->xyz_own = own;
    return rc;
  }
  if (f->n_store > 0)
    HIP_TRY(ctx, hipMemcpyAsync(own.p, f->xyz.p, (size_t)f->n_store * 24, hipMemcpyDeviceToDevice, ctx->stream));
  f->xyz = own;
  f->store_borrowed = false;
  return OCTL_OK;
}

// the n points just appended to the store become a new pose (its slot: the number of poses before it)
static int commit_new_pose(octl_forest* f, int64_t n, int32_t* slot) {
  if (slot) *slot = (int32_t)f->pose_off.size() - 1;
  f->n_store += n;
  f->n_alive += n;
  f->pose_off.push_back(f->n_store);
  f->store_dirty = true;
  forest_contents_changed(f);
  return OCTL_OK;
}

static int extend_pose_impl(octl_forest* f, int32_t slot, const void* xyz, int64_t n, bool from_device,
                            bool f32 = false, const XfArgs* xf = nullptr) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (xf) OCTL_TRY(xf_args_check(ctx, *xf, xyz, n));
  const int n_poses = (int)f->pose_off.size() - 1;
  if (slot < 0 || slot >= n_poses) return octl_set_error(ctx, OCTL_E_INVALID, "bad pose slot");
  const int64_t tail = f->n_store - f->pose_off[slot + 1];  // points of the later poses
  // (a device cloud may be the target of an octl_dev_upload_async that is still in flight)
  if (from_device && n > 0) OCTL_TRY(ctx_wait_uploads(ctx, xyz, (size_t)n * (f32 ? 12 : 24)));
  // lands behind everything (bounding box, alive flags)
  if (xf) {
    OCTL_TRY(store_append_xf(f, xyz, n, *xf));
  } else if (f32) {
    OCTL_TRY(store_append_f32(f, static_cast<const float*>(xyz), n, from_device));
  } else {
    OCTL_TRY(store_append(f, static_cast<const double*>(xyz), n, from_device));
  }
  if (tail > 0 && n > 0) {
    // The store is pose-major: rotate the new points in front of the later poses' points (they were
    // appended at the end).  The whole range [tail | new] goes through the partition scratch and comes
    // back as [new | tail]: with more new points than later points the two pieces overlap in the
    // store, so nothing is copied store-to-store.  The next build re-derives every table from the store.
    hipStream_t st = ctx->stream;
    const int64_t at = f->pose_off[slot + 1];
    const int64_t span = tail + n;
    OCTL_TRY(devbuf_reserve(ctx, f->part_xyz[0], (size_t)span * 25));
    char* tmp = static_cast<char*>(f->part_xyz[0].p);
    char* tmp_al = tmp + (size_t)span * 24;
    double* xs = f->xyz.as<double>();
    uint8_t* al = f->alive.as<uint8_t>();
    HIP_TRY(ctx, hipMemcpyAsync(tmp, xs + 3 * at, (size_t)span * 24, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(tmp_al, al + at, (size_t)span, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(xs + 3 * at, tmp + (size_t)tail * 24, (size_t)n * 24, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(al + at, tmp_al + tail, (size_t)n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(xs + 3 * (at + n), tmp, (size_t)tail * 24, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(al + at + n, tmp_al, (size_t)tail, hipMemcpyDeviceToDevice, st));
  }
  f->n_store += n;
  f->n_alive += n;
  for (int p = slot + 1; p <= n_poses; ++p) f->pose_off[p] += n;
  f->store_dirty = true;
  forest_contents_changed(f);
  f->append_only = false;  // the store was rotated: the next build re-places everything
  return OCTL_OK;
}

extern "C" {

int octl_forest_add_pose(octl_forest* f, const double* xyz, int64_t n, int32_t* slot) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  OCTL_TRY(store_append(f, xyz, n, false));
  return commit_new_pose(f, n, slot);
}

int octl_forest_add_pose_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t* slot) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  // (the cloud may be the target of an octl_dev_upload_async that is still in flight)
  if (n > 0) OCTL_TRY(ctx_wait_uploads(f->ctx, xyz_dev, (size_t)n * 24));
  OCTL_TRY(store_append(f, xyz_dev, n, true));
  return commit_new_pose(f, n, slot);
}

int octl_forest_add_pose_f32(octl_forest* f, const float* xyz, int64_t n, int32_t* slot) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  OCTL_TRY(store_append_f32(f, xyz, n, false));
  return commit_new_pose(f, n, slot);
}

int octl_forest_add_pose_device_f32(octl_forest* f, const float* xyz_dev, int64_t n, int32_t* slot) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  // (the cloud may be the target of an octl_dev_upload_async that is still in flight)
  if (n > 0) OCTL_TRY(ctx_wait_uploads(f->ctx, xyz_dev, (size_t)n * 12));
  OCTL_TRY(store_append_f32(f, xyz_dev, n, true));
  return commit_new_pose(f, n, slot);
}

int octl_forest_add_pose_xf(octl_forest* f, const void* xyz, int64_t n, uint32_t flags, const double* transforms,
                            int32_t n_transforms, const uint16_t* segment, int32_t* slot) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  const XfArgs a{flags, transforms, n_transforms, segment};
  OCTL_TRY(xf_args_check(f->ctx, a, xyz, n));
  // (the cloud may be the target of an octl_dev_upload_async that is still in flight)
  if (a.device() && n > 0) OCTL_TRY(ctx_wait_uploads(f->ctx, xyz, (size_t)n * (a.f32() ? 12 : 24)));
  OCTL_TRY(store_append_xf(f, xyz, n, a));
  return commit_new_pose(f, n, slot);
}

int octl_forest_add_pose_adopt(octl_forest* f, const double* xyz_dev, int64_t n, int32_t* slot) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  // only the first pose of an empty forest can be read in place (the store is one contiguous array); the
  // kernels read 16 bytes at a time from the start of the cloud
  if (f->n_store != 0 || n <= 0 || !xyz_dev || (reinterpret_cast<uintptr_t>(xyz_dev) & 15) != 0)
    return octl_forest_add_pose_device(f, xyz_dev, n, slot);
  // (the cloud may be the target of an octl_dev_upload_async that is still in flight)
  OCTL_TRY(ctx_wait_uploads(f->ctx, xyz_dev, (size_t)n * 24));
  if (!f->store_borrowed) f->xyz_own = f->xyz;
  f->xyz = DevBuf{const_cast<double*>(xyz_dev), 0};
  f->store_borrowed = true;
  const int rc = store_take_in_place(f, n);
  if (rc != OCTL_OK) {
    f->xyz = f->xyz_own;
    f->xyz_own = DevBuf{};
    f->store_borrowed = false;
    return rc;
  }
  return commit_new_pose(f, n, slot);
}

int octl_forest_transform_poses(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, const double* transforms) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  const int n_poses = (int)f->pose_off.size() - 1;
  int S = 0;
  for (int s = 0; s < n_poses; ++s) S += (sel.empty() || sel[s]) ? 1 : 0;
  if (S > 0 && !transforms) return octl_set_error(ctx, OCTL_E_INVALID, "transform_poses: null transforms");
  for (int k = 0; k < 12 * S; ++k)
    if (!std::isfinite(transforms[k]))
      return octl_set_error(ctx, OCTL_E_INVALID, "transform_poses: the transform of selected pose %d is not finite",
                            k / 12);
  const int64_t n = f->n_store;
  if (S == 0 || n == 0) return OCTL_OK;  // (nothing moves: the forest, built or not, stays as it is)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // The moved store is written OUT of place, so that a call that fails leaves every byte the forest reads where it
  // was: into the forest's own block while the store is the caller's buffer (never written), else into the first
  // partition scratch of the bucket build, which then swaps with the store (a bucket build leaves 32 bytes per point
  // there and a swapped-out store block holds the store: neither grows here again).  Every allocation comes before
  // the first launch.
  DevBuf& target = f->store_borrowed ? f->xyz_own : f->part_xyz[0];
  OCTL_TRY(devbuf_reserve(ctx, target, (size_t)n * 24 + 16));
  const XfLayout lay(n_poses);
  OCTL_TRY(devbuf_reserve(ctx, f->xf_tab, lay.plan.total));
  OCTL_TRY(devbuf_reserve(ctx, f->bbox_dev, 32));
  std::vector<char> host(lay.plan.total, 0);
  {
    int32_t* box = reinterpret_cast<int32_t*>(host.data() + lay.box.off);
    for (int a = 0; a < 8; ++a) box[a] = a < 3 ? (1 << 30) : (a < 6 ? -(1 << 30) : 0);
    std::memcpy(host.data() + lay.end.off, f->pose_off.data() + 1, (size_t)n_poses * 8);
    XfSlot* slot = reinterpret_cast<XfSlot*>(host.data() + lay.slot.off);
    for (int s = 0, k = 0; s < n_poses; ++s) {
      if (!(sel.empty() || sel[s])) continue;
      std::memcpy(slot[s].m, transforms + 12 * (size_t)k++, sizeof slot[s].m);
      slot[s].selected = 1;
    }
  }
  HIP_TRY(ctx, hipMemcpyAsync(f->xf_tab.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
  int32_t* box_d = Carve::at(f->xf_tab, lay.box);
  {
    KTimer t(ctx, "transform_poses");
    OCTL_LAUNCH(k_transform_poses, dim3((unsigned)ceil_div(n, XF_ROWS_PER_WG)), dim3(256), 0, st,
                (const double*)f->xyz.as<double>(), target.as<double>(),
                f->alive_stale ? (const uint8_t*)nullptr : (const uint8_t*)f->alive.as<uint8_t>(), n,
                (const int64_t*)Carve::at(f->xf_tab, lay.end), (const XfSlot*)Carve::at(f->xf_tab, lay.slot), n_poses,
                f->mode, f->edge, f->corner[0], f->corner[1], f->corner[2], box_d);
    HIP_TRY(ctx, hipGetLastError());
  }
  // the one host wait: the box and the domain flag through the context's mirror (also: `host` is ours again)
  int32_t bb[8];
  {
    int32_t* mirror = reinterpret_cast<int32_t*>(static_cast<char*>(ctx->small_host) + MIRROR_BBOX_WORD * 4);
    HIP_TRY(ctx, hipMemcpyAsync(mirror, box_d, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::memcpy(bb, mirror, sizeof bb);
  }
  if (bb[6])  // (the output is dropped where it lies: scratch, or the forest's idle own block)
    return octl_set_error(ctx, OCTL_E_DOMAIN,
                          "transform_poses: a moved point %s; the map is unchanged",
                          f->mode == 0 ? "has a non-finite coordinate or a top-level voxel index outside +-2^30"
                                       : "lies outside the cube or is not finite");
  // ---- commit: the moved store, the box just folded, and a forest without a scheme --------------------------------
  HIP_TRY(ctx, hipMemcpyAsync(f->bbox_dev.p, box_d, 32, hipMemcpyDeviceToDevice, st));
  if (f->store_borrowed) {
    f->xyz = f->xyz_own;
    f->xyz_own = DevBuf{};
    f->store_borrowed = false;
  } else {
    std::swap(f->xyz, f->part_xyz[0]);
  }
  f->bbox_stale = f->bbox_pending = false;
  forest_reset_scheme(f);
  return OCTL_OK;
}

int octl_forest_remove_poses(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int32_t* new_slot,
                             int64_t* n_removed) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  const int n_poses = (int)f->pose_off.size() - 1;
  // shifts, new slots (dense, ascending) and new offsets
  std::vector<int64_t> shift((size_t)n_poses + 1, 0), off_new(1, 0);
  std::vector<int32_t> slot_new((size_t)std::max(n_poses, 1), -1);
  int S = 0;
  for (int s = 0; s < n_poses; ++s) {
    const bool leaves = sel.empty() || sel[s];
    const int64_t size = f->pose_off[s + 1] - f->pose_off[s];
    shift[s + 1] = shift[s] + (leaves ? size : 0);
    if (leaves) {
      ++S;
    } else {
      slot_new[s] = (int32_t)off_new.size() - 1;
      off_new.push_back(off_new.back() + size);
    }
  }
  if (S == 0) {  // (nothing leaves: no launch, no state change)
    if (n_removed) *n_removed = 0;
    if (new_slot)
      for (int s = 0; s < n_poses; ++s) new_slot[s] = s;
    return OCTL_OK;
  }
  if (f->built && f->store_dirty)
    return octl_set_error(ctx, OCTL_E_STATE,
                          "remove_poses: points were added since the forest was built (bring it up to date first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t n_old = f->n_store, n_new = n_old - shift[n_poses];
  const bool tables = f->built && !f->store_dirty;
  // ---- every buffer before anything the forest reads is changed: a failed allocation leaves it as it was ---------
  DevBuf& target = f->store_borrowed ? f->xyz_own : f->part_xyz[0];
  if (n_new > 0) {
    OCTL_TRY(devbuf_reserve(ctx, target, (size_t)n_new * 24 + 16));
    OCTL_TRY(devbuf_reserve(ctx, f->alive2, (size_t)n_new + 2));
  }
  const RetireLayout lay(n_poses);
  OCTL_TRY(devbuf_reserve(ctx, f->xf_tab, lay.plan.total));
  OCTL_TRY(devbuf_reserve(ctx, f->bbox_dev, 32));
  if (tables) OCTL_TRY(mask_retire_reserve(f));
  std::vector<char> host(lay.plan.total, 0);
  {
    int32_t* box = reinterpret_cast<int32_t*>(host.data() + lay.box.off);
    for (int a = 0; a < 8; ++a) box[a] = a < 3 ? (1 << 30) : (a < 6 ? -(1 << 30) : 0);
    std::memcpy(host.data() + lay.end.off, f->pose_off.data() + 1, (size_t)n_poses * 8);
    std::memcpy(host.data() + lay.shift.off, shift.data(), ((size_t)n_poses + 1) * 8);
    std::memcpy(host.data() + lay.new_slot.off, slot_new.data(), (size_t)n_poses * 4);
    uint8_t* sel_h = reinterpret_cast<uint8_t*>(host.data() + lay.sel.off);
    for (int s = 0; s < n_poses; ++s) sel_h[s] = (sel.empty() || sel[s]) ? 1 : 0;
  }
  HIP_TRY(ctx, hipMemcpyAsync(f->xf_tab.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
  int32_t* box_d = Carve::at(f->xf_tab, lay.box);
  unsigned long long* cnt_d = reinterpret_cast<unsigned long long*>(box_d + 8);
  const int64_t* shift_d = Carve::at(f->xf_tab, lay.shift);
  const int64_t alive_before = f->n_alive;
  // the removed poses' blocks leave the leaf-ordered arrays and the block table (with a pending RANSAC mask, in the
  // same compaction); the alive flags are cleared by OLD store index: before the store pass
  if (tables) OCTL_TRY(mask_retire_slots(f, Carve::at(f->xf_tab, lay.sel), cnt_d));
  {
    KTimer t(ctx, "remove_poses");  // (with k_retire_mask's: the compaction between them keeps its own label)
    if (tables) {
      if (f->n_blocks > 0) {
        OCTL_LAUNCH(k_retire_blocks, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st,
                    (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                    f->blk_slot.as<int32_t>(), f->n_blocks, shift_d, (const int32_t*)Carve::at(f->xf_tab, lay.new_slot),
                    f->ord_idx.as<uint32_t>());
        HIP_TRY(ctx, hipGetLastError());
      }
    }
    if (n_new > 0) {
      const bool flags = !f->alive_stale;
      OCTL_LAUNCH(k_retire_poses, dim3((unsigned)ceil_div(n_new, RT_ROWS_PER_WG)), dim3(256), 0, st,
                  (const double*)f->xyz.as<double>(), target.as<double>(),
                  flags ? (const uint8_t*)f->alive.as<uint8_t>() : (const uint8_t*)nullptr,
                  flags ? f->alive2.as<uint8_t>() : (uint8_t*)nullptr, n_new,
                  (const int64_t*)Carve::at(f->xf_tab, lay.end), shift_d, n_poses, f->mode, f->edge, box_d);
      HIP_TRY(ctx, hipGetLastError());
      // (with tables the compaction has booked the rows that left; without, the flags just written are counted)
      if (!tables && flags) {
        OCTL_LAUNCH(k_alive_count, dim3((unsigned)std::min<int64_t>(ceil_div(n_new, 256 * 16 * 8), 256)), dim3(256), 0,
                    st, (const uint8_t*)f->alive2.as<uint8_t>(), n_new, cnt_d + 1);
        HIP_TRY(ctx, hipGetLastError());
      }
    }
  }
  // the call's own host wait: its two counters through the context's mirror (also: `host` is ours again)
  unsigned long long cnt[2];
  {
    char* mirror = static_cast<char*>(ctx->small_host) + MIRROR_BBOX_WORD * 4;
    HIP_TRY(ctx, hipMemcpyAsync(mirror, cnt_d, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::memcpy(cnt, mirror, sizeof cnt);
  }
  // ---- commit: the squeezed store with its flags, the box just folded, the poses renumbered ----------------------
  HIP_TRY(ctx, hipMemcpyAsync(f->bbox_dev.p, box_d, 32, hipMemcpyDeviceToDevice, st));
  if (f->store_borrowed) {  // (the caller's buffer was only read; with no pose left nothing was written at all)
    f->xyz = f->xyz_own;
    f->xyz_own = DevBuf{};
    f->store_borrowed = false;
  } else if (n_new > 0) {
    std::swap(f->xyz, f->part_xyz[0]);
  }
  if (n_new > 0 && !f->alive_stale) std::swap(f->alive, f->alive2);
  if (n_new == 0) f->alive_stale = false;
  f->bbox_stale = f->bbox_pending = false;
  f->pose_off = off_new;
  f->pose_off_uploaded.clear();
  f->n_store = n_new;
  if (!tables) f->n_alive = f->alive_stale ? n_new : (int64_t)cnt[1];  // (flags never written: every row alive)
  if (n_removed) *n_removed = tables ? (int64_t)cnt[0] : alive_before - f->n_alive;
  f->built_store = tables ? n_new : 0;
  f->built_poses = tables ? (int)off_new.size() - 1 : 0;
  f->fast_order_valid = false;
  // (the selections the derived tables were made for count poses that are gone)
  f->pl_stamp = f->adj_stamp = f->nn_stamp = f->seg_stamp = 0;
  f->pl_sel.clear();
  f->adj_sel.clear();
  f->adj_slots.clear();
  f->adj_chunk_off.clear();
  f->adj_called = false;
  f->nn_sel.clear();
  f->seg_sel.clear();
  forest_contents_changed(f);
  if (new_slot) std::memcpy(new_slot, slot_new.data(), (size_t)n_poses * 4);
  return OCTL_OK;
}

int octl_forest_store_size(octl_forest* f, int64_t* n_store, int64_t* n_alive, int32_t* n_poses) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  if (n_store) *n_store = f->n_store;
  if (n_alive) *n_alive = f->n_alive;
  if (n_poses) *n_poses = (int32_t)f->pose_off.size() - 1;
  return OCTL_OK;
}

int octl_forest_extend_pose(octl_forest* f, int32_t slot, const double* xyz, int64_t n) {
  return extend_pose_impl(f, slot, xyz, n, false);
}

int octl_forest_extend_pose_device(octl_forest* f, int32_t slot, const double* xyz_dev, int64_t n) {
  return extend_pose_impl(f, slot, xyz_dev, n, true);
}

int octl_forest_extend_pose_f32(octl_forest* f, int32_t slot, const float* xyz, int64_t n) {
  return extend_pose_impl(f, slot, xyz, n, false, true);
}

int octl_forest_extend_pose_device_f32(octl_forest* f, int32_t slot, const float* xyz_dev, int64_t n) {
  return extend_pose_impl(f, slot, xyz_dev, n, true, true);
}

int octl_forest_extend_pose_xf(octl_forest* f, int32_t slot, const void* xyz, int64_t n, uint32_t flags,
                               const double* transforms, int32_t n_transforms, const uint16_t* segment) {
  const XfArgs a{flags, transforms, n_transforms, segment};
  return extend_pose_impl(f, slot, xyz, n, a.device(), a.f32(), &a);
}

}  // extern "C"
