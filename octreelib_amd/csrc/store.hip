// The point store of a forest: the ingest kernels that copy (or widen) a pose into it, mark its points alive and
// fold their voxel box, and the C entries that add or extend poses.
#include "forest.h"
#include "ref_arith.h"

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
                            bool f32 = false) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  const int n_poses = (int)f->pose_off.size() - 1;
  if (slot < 0 || slot >= n_poses) return octl_set_error(ctx, OCTL_E_INVALID, "bad pose slot");
  const int64_t tail = f->n_store - f->pose_off[slot + 1];  // points of the later poses
  // (a device cloud may be the target of an octl_dev_upload_async that is still in flight)
  if (from_device && n > 0) OCTL_TRY(ctx_wait_uploads(ctx, xyz, (size_t)n * (f32 ? 12 : 24)));
  // lands behind everything (bounding box, alive flags)
  if (f32) {
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

}  // extern "C"
