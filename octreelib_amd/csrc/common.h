// Shared host-side infrastructure of liboctree_hip.so: context, device buffers, error
// plumbing, per-kernel hipEvent timers.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/octreelib_hip.h"

// Every place where the host waits for the device is counted (octl_debug_host_syncs): the number of
// round trips per step is part of what bench.py reports.
#include <atomic>
extern std::atomic<uint64_t> g_octl_host_syncs;
static inline hipError_t octl_counted_stream_sync(hipStream_t s) {
  g_octl_host_syncs.fetch_add(1, std::memory_order_relaxed);
  return hipStreamSynchronize(s);
}
static inline hipError_t octl_counted_event_sync(hipEvent_t e) {
  g_octl_host_syncs.fetch_add(1, std::memory_order_relaxed);
  return hipEventSynchronize(e);
}
#define hipStreamSynchronize(s) octl_counted_stream_sync(s)
#define hipEventSynchronize(e) octl_counted_event_sync(e)
// ... and every kernel launch and asynchronous fill (a fill is a kernel of the runtime's): octl_debug_launches -
// launches per step is the other figure a small scan lives by
extern std::atomic<uint64_t> g_octl_launches;
// ... and everything the library puts on a stream - launches, fills and copies (not part of any reported figure): what
// a context compares its own tally of harmless work against before a build runs ahead (octl_ctx::ahead_*)
extern std::atomic<uint64_t> g_octl_enqueues;
// builds whose partition front ran on the context's ahead stream (octl_debug_builds_ahead)
extern std::atomic<uint64_t> g_octl_builds_ahead;
// speculative launches of k_bucket_finish that did the work / that the host had to repeat (octl_debug_spec_finish)
extern std::atomic<uint64_t> g_octl_spec_held, g_octl_spec_missed;
// (the project's own launch macro around the PUBLIC hipLaunchKernelGGL - not a redefinition of the runtime's macro
//  through its internals: a ROCm update that renames those would break every translation unit)
#define OCTL_LAUNCH(...)                                                      \
  do {                                                                        \
    g_octl_launches.fetch_add(1, std::memory_order_relaxed);                  \
    g_octl_enqueues.fetch_add(1, std::memory_order_relaxed);                  \
    hipLaunchKernelGGL(__VA_ARGS__);                                          \
  } while (0)
#define hipMemsetAsync(...)                                                                                      \
  (g_octl_launches.fetch_add(1, std::memory_order_relaxed), g_octl_enqueues.fetch_add(1, std::memory_order_relaxed), \
   hipMemsetAsync(__VA_ARGS__))
#define hipMemcpyAsync(...) (g_octl_enqueues.fetch_add(1, std::memory_order_relaxed), hipMemcpyAsync(__VA_ARGS__))

// Compile-time experiment switches that change RESULTS (ablations, duplicated work) or add instrumentation never
// belong in a shipped library: they only compile when the variant build script defines OCTL_EXPERIMENTS
// (tools/build_variant.sh -> build/variants/NAME.so, loaded through OCTREELIB_AMD_LIB; the Makefile never does).
#if !defined(OCTL_EXPERIMENTS) && \
    (defined(PS_DUP_KEYS) || defined(PS_DUP_STORE) || defined(RS_COUNTS) || defined(BB_STAMPS))
#error "PS_DUP_* / RS_COUNTS / BB_STAMPS are experiments: build them with tools/build_variant.sh (-DOCTL_EXPERIMENTS)"
#endif

#define OCTL_WAVE 64
#define OCTL_PINNED_BYTES (256 * 1024)

struct KernelTiming {
  double ms = 0.0;
  int64_t launches = 0;
};

struct PendingEvent {
  std::string name;
  hipEvent_t start, stop;
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

// Diagnostic switches of a context (tests and A/B runs compare code paths with them).  Read from the environment
// ONCE, when the context is created (OCTL_<NAME>=value), or set afterwards with octl_debug_set_option; nothing on a
// build's path calls getenv.  All default to 0 = the shipped behaviour.
struct OctlOptions {
  int64_t no_bucket_build = 0;     // OCTL_NO_BUCKET_BUILD: every build through the level-synchronous path
  int64_t bucket_points = 0;       // OCTL_BUCKET_POINTS: average points per bucket (0: 2560; 1280 up to 400 k points)
  int64_t sync_geom = 0;           // OCTL_SYNC_GEOM: the host-side form of the key geometry on small clouds too
  int64_t no_geom_hint = 0;        // OCTL_NO_GEOM_HINT: no geometry carried over from the context's previous build
  int64_t no_exact_digits = 0;     // OCTL_NO_EXACT_DIGITS: child digits level by level, never six at once
  int64_t no_fast_order = 0;       // OCTL_NO_FAST_ORDER: the listing order always from order.hip
  int64_t no_bucket_history = 0;   // OCTL_NO_BUCKET_HISTORY: a subdivide over a previous scheme through the general path
  int64_t no_cube_fast = 0;        // OCTL_NO_CUBE_FAST: a fresh single cube through key generation
  int64_t no_cube_prefix = 0;      // OCTL_NO_CUBE_PREFIX: no prefix partition of big single cubes
  int64_t cube_prefix_min = 0;     // OCTL_CUBE_PREFIX_MIN: points from which a single cube is prefix-partitioned (0: 4 Mi)
  int64_t no_incremental = 0;      // OCTL_NO_INCREMENTAL: late poses by re-placement of every stored point
  int64_t route_self_sendrecv = 0; // OCTL_ROUTE_SELF_SENDRECV: a rank's own part through RCCL too (1-rank rehearsal)
  int64_t trace_build = 0;         // OCTL_TRACE_BUILD: host wall time between the phases of forest_build on stderr
  int64_t scan_mode = 0;           // OCTL_SCAN: 1 = single-pass scan always, 3 = three-kernel scan always
  int64_t no_fused_tables = 0;     // OCTL_NO_FUSED_TABLES: the small table chains as separate launches (A/B)
  int64_t no_spin_wait = 0;        // OCTL_NO_SPIN_WAIT: every host wait is a hipStreamSynchronize (A/B)
  int64_t ransac_waves = 0;        // OCTL_RANSAC_WAVES: waves per block of the H > 256 RANSAC instances (0: the library's policy; 1, 2, 4)
  int64_t geom_margin = 0;         // OCTL_GEOM_MARGIN: voxels of slack around the true box in a single-pass / hinted key geometry (0: one voxel; negative: none)
  int64_t no_ransac_prescreen = 0; // OCTL_NO_RANSAC_PRESCREEN: every hypothesis of a leaf through the exact plane fit (no approximate prescreen)
  int64_t no_spec_finish = 0;      // OCTL_NO_SPEC_FINISH: k_bucket_finish only behind the host's look at the totals (A/B)
  int64_t no_build_ahead = 0;      // OCTL_NO_BUILD_AHEAD: the partition front of a build never on the ahead stream (A/B)
  // OCTL_BUILD_AHEAD_MIN_POINTS: points from which a build may run ahead (unset: OCTL_AHEAD_MIN_POINTS; 0: every size)
  int64_t build_ahead_min_points = -1;
};
// name (without the OCTL_ prefix or with it) -> field; nullptr when there is no such switch
int64_t* octl_option_field(OctlOptions& o, const char* name);

struct octl_ctx {
  int device = 0;
  OctlOptions opt;
  hipStream_t stream = nullptr;
  std::string err;
  int profiling = 0;  // 0 off, 1 every timed region, 2 the RANSAC kernel only (an event pair costs ~10 us of pipeline)
  std::map<std::string, KernelTiming> timings;
  std::vector<PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
  // scratch for scans / sorts (grown on demand, reused across calls)
  DevBuf scan_tmp[3];
  DevBuf scan_status;            // single-pass scan: per-tile status words
  uint32_t scan_epoch = 0;
  int cus = 0;      // compute units of the device (queried once: hipGetDeviceProperties is not free)
  DevBuf small;     // 4 KiB of device scalars (counters, flags)
  void* small_host = nullptr;  // pinned mirror
  void* pinned = nullptr;      // pinned staging for small uploads (OCTL_PINNED_BYTES)
  // one event per staging region ([0,128K) build, [128K,192K) hypothesis table, [192K,256K) pose
  // epochs): recorded after the region's H2D copy, waited for before the region is written again
  hipEvent_t pin_event[3] = {nullptr, nullptr, nullptr};
  hipEvent_t handoff_event = nullptr;  // orders a buffer handed to another context behind this stream
  // asynchronous host feed (octl_dev_upload_async): a second stream for host-to-device copies, so that the
  // upload of scan i+1 overlaps the build and fit of scan i; copy_gate orders a copy behind the compute work
  // enqueued before it (its destination may still be read), copy_done orders compute behind the copies
  hipStream_t copy_stream = nullptr;
  hipEvent_t copy_gate = nullptr;
  // The context's SIDE stream (octl_ctx_side_stream): work that may run next to the context's stream between two
  // events - self_gate: what it reads is complete on the context's stream; self_done: the side work is.
  // route.hip: a rank's own part of the all-to-all, next to the RCCL transfers; ransac.hip: the instances for the
  // larger blocks of a split launch, next to the one-wave instance.
  hipStream_t self_stream = nullptr;
  hipEvent_t self_gate = nullptr, self_done = nullptr;
  // The context's AHEAD stream (octl_ctx_ahead_stream): the partition front of a build - k_build_begin,
  // k_part_hist<true,*>, k_table_scan, k_part_scatter, the pose offsets' copy - next to the RANSAC and the mask of the
  // context's PREVIOUS scan, which are still in flight on the context's stream.
  //   ahead_free   recorded on the context's stream behind a build's last launch (by the first allow-listed function
  //                that follows it, in front of its own work): the front's scratch is free;
  //                the ahead stream waits for it (and for the uploads into the cloud) and for nothing else
  //   ahead_done   recorded behind the front; the context's stream waits for it in front of k_bucket_build (the JOIN,
  //                octl_ahead_join - on every path out of forest_build once ahead_open is set)
  // A build runs ahead only when, since ahead_free, the library enqueued nothing on this context but work that
  // touches none of the front's memory (AheadAllow): g_octl_enqueues == ahead_mark + ahead_allowed.
  hipStream_t ahead_stream = nullptr;
  hipEvent_t ahead_free = nullptr, ahead_done = nullptr;
  DevBuf ahead_status;               // look-back status words of the front's k_table_scan (OCTL_AHEAD_TILES), with
  uint32_t ahead_epoch = 0;          // an epoch counter of their own: the context's belong to chains on its stream
  int ahead_allow_depth = 0;         // AheadAllow scopes that are open (only the outermost one counts)
  bool ahead_open = false;           // a front is on the ahead stream and the context's stream has not joined it yet
  bool ahead_mark_pending = false;   // a build of ahead_forest succeeded; ahead_free is still to be recorded (octl_ahead_arm)
  bool ahead_mark_valid = false;     // ahead_free stands behind that build, with nothing but allow-listed work behind it
  const struct octl_forest* ahead_forest = nullptr;
  uint64_t ahead_mark = 0, ahead_allowed = 0;
  struct Upload { const char* dst; size_t bytes; hipEvent_t done; };
  std::vector<Upload> uploads;  // copies that may still be in flight, each with the event recorded behind it
  // device blocks handed back by destroyed forests, kept for the next one: a fresh Grid per scan
  // otherwise pays ~10 ms of hipMalloc / hipFree per build for its dozen large buffers
  std::vector<DevBuf> pool;
  size_t pool_bytes = 0;
  // blocks handed out by octl_dev_alloc (pointer -> capacity): they come from and go back to the pool too - a
  // hipMalloc / hipFree pair of a 240 MB scan buffer costs milliseconds and synchronises the device
  std::map<void*, size_t> user_blocks;
  // key geometry (padded voxel box, bucket width) formed from the TRUE box of the last bucket build on this context:
  // the next build of a cloud that was taken in place starts its histogram pass under this geometry and finds its own
  // true box in the same pass (bucket_build.hip: hinted geometry); opaque here
  unsigned char geom_hint[192] = {0};
  bool geom_hint_valid = false;
  bool geom_hint_staged = false;  // forest_build's first launch has put the hint into the scalar block already
  struct octl_forest* pending_mask_forest = nullptr;  // the forest whose apply_mask totals are still in flight (one per context: they share the mirror's words)
  uint64_t geom_hint_want = 0;
  bool geom_hint_two_pass = false;  // the hint is the geometry of a TWO-pass build (> 4096 buckets, host-side form)
  // the last build found a sparse scene (more than 4096 buckets): the next one skips the single-pass attempt
  bool geom_sparse = false;
  // the last bucket build had buckets beyond 4096 points (a skewed scene): the next one launches the chunk kernels
  // beside k_bucket_build right away instead of learning about them from the totals (two launches an even scene saves)
  bool had_chunks = false;
  // node / voxel / block counts of the context's previous bucket build: the tables of a speculative k_bucket_finish
  // are sized from them (0: no bucket build yet)
  int64_t spec_points = 0, spec_nodes = 0, spec_vox = 0, spec_blocks = 0;
  // the hypothesis table of the last octl_forest_ransac_all on this context (CudaRansac draws it once per object,
  // cuda_ransac.py:39-41, and a loop over scans hands the same one over for every scan - to a fresh forest each
  // time): kept per CONTEXT so that it is uploaded once
  DevBuf hyp_dev;
  // device staging of host float32 clouds (octl_forest_add_pose_f32 / _extend_pose_f32): the upload lands here and
  // the ingest kernel widens it into the forest's f64 store; kept between calls so that a scan loop does no hipMalloc
  DevBuf f32_stage;
  // clouds inserted under a transform (octl_forest_*_pose_xf): device staging of the transform table and the segment
  // indices; for a DEVICE cloud, whose call does not wait, they are uploaded from xf_host - the library's copy of the
  // caller's arrays - and xf_event, recorded behind that upload, is waited for before xf_host is written again
  DevBuf xf_stage;
  std::vector<char> xf_host;
  hipEvent_t xf_event = nullptr;
  bool xf_inflight = false;
  // octl_forest_leaf_stats / octl_debug_sym3_eigen (leaf_stats.hip): block ids, outputs, claim words, chunk work
  // items and chunk partials of one call; kept between calls
  DevBuf ls_buf;
  // launch counters of ransac.hip's preparation: two sets used alternately (a launch zeroes the next one's)
  DevBuf rs_counters;
  int rs_parity = 0;
  uint32_t wait_seq = 0;   // sequence numbers of the mirror flags (octl_wait_mirror_flags)
  bool rs_counters_dirty = false;
  std::vector<double> hyp_host;
  // RCCL (route.hip)
  void* comm = nullptr;
  int n_ranks = 1, rank = 0;
  // routed cloud of the last octl_route_points + its scratch (kept: hipMalloc per step costs ms)
  DevBuf routed_xyz, routed_gidx;
  bool routed_taken = false;  // a forest took routed_xyz over: nothing to hand out until the next route
  DevBuf rt_hist, rt_counts, rt_matrix, rt_send_xyz, rt_send_gidx;
  int64_t routed_n = 0;
};

int octl_set_error(octl_ctx* ctx, int code, const char* fmt, ...);
// Host waits for a few scalars, not for the stream: the kernel that produces them writes them into the pinned mirror
// (ctx->small_host) and then the launch's sequence number into flag word(s) of that mirror; the host polls the flags
// for up to budget_us and only then falls back to hipStreamSynchronize.  (A stream synchronisation returns 15-25 us
// after the kernel has finished - interrupt, wake-up - which is a tenth of a 100 k-point scan.)  Counted as a host
// wait like a synchronisation.  Words of the mirror: MIRROR_FLAG_BUILD (bucket totals), MIRROR_FLAG_MASK0/1
// (apply_mask: kept points, surviving blocks), MIRROR_MASK_TOTALS (the two totals themselves).
// Layout of the 4 KB mirror (words): [0, MIRROR_COPY_WORDS) targets of small device-to-host copies and the scalar
// block a build mirrors; MIRROR_BBOX_WORD.. the voxel box read back by the host-side geometry; then the words above,
// which no copy may reach.
// MIRROR_RS_VIOLATION: set by ransac.hip's preparation kernel when a block is larger than the launch was told any
// block could be (max_block: the instances for larger blocks are not launched then) - every host wait checks it.
enum { MIRROR_COPY_WORDS = 512, MIRROR_BBOX_WORD = 896, MIRROR_RS_VIOLATION = 990, MIRROR_MASK_TOTALS = 992,
       MIRROR_FLAG_BUILD = 1000, MIRROR_FLAG_MASK0 = 1001, MIRROR_FLAG_MASK1 = 1002 };
static_assert(MIRROR_COPY_WORDS <= MIRROR_BBOX_WORD && MIRROR_BBOX_WORD + 8 <= MIRROR_RS_VIOLATION &&
              MIRROR_RS_VIOLATION < MIRROR_MASK_TOTALS &&
              MIRROR_MASK_TOTALS + 2 <= MIRROR_FLAG_BUILD && MIRROR_FLAG_MASK1 < 1024, "mirror layout");
// Words of the context's scalar block ctx->small (4 KiB of device uint32; the pinned mirror above has the same size).
// Who may write what, now that the partition front of a build can run on the ahead stream NEXT TO the RANSAC and the
// apply_mask of the context's previous scan:
//  - the FRONT's words: [0, SM_BUILD_WORDS), which forest_build's first kernel (k_build_begin) resets, and the key
//    geometry SM_GEOM.. (staged by k_build_begin, validated by k_table_scan / k_part_scatter).  Work that may be in
//    flight beside a front - ransac_launch, apply_mask, the hypothesis table's upload (the functions that hold an
//    AheadAllow) - owns NO word in these ranges: SM_MASK_TOTAL lies behind them, ransac_launch uses none at all.
//  - every other name in the front's ranges belongs to a build itself or to an operation that is not on that list;
//    such an operation makes the context's next build serial (octl_ctx::ahead_mark), so it is never in flight beside
//    a front.  Among them a word with more than one name has owners that never hold a live value at the same time:
//    28..31: the bucket build (SM_BK_MISSING, SM_CK_COUNT), the incremental insertion (SM_INC_*) and
//    octl_forest_slot_counts (SM_SLOT_COUNTS).  forest_build tries the incremental insertion first and falls through
//    to the bucket build only for K < 0 over a scheme without internal nodes: k_inc_place then never counts SM_INC_BAD
//    (it counts only in cubes that are split), so word 29 still holds the zero SM_CK_COUNT starts from, and the bucket
//    build zeroes word 28 itself before k_old_voxels_missing counts into it.  build.hip's prefix partition counts
//    into SM_BK_MISSING only on a forest that was never built, which the incremental insertion leaves alone.
//    octl_forest_slot_counts zeroes its four words and reads them back before it returns: never inside a build.
//  - SM_SLOT_HIST (the reference order of a RANSAC pass over several poses) has words of its own behind SM_GEOM: it
//    shared them with the geometry while a build and a RANSAC pass could not overlap.
enum {
  SM_ERR = 0,           // domain error flag
  SM_BBOX = 4,          // 6 x int32: min xyz, max xyz
  SM_NVOX = 12,         // voxels with points
  SM_NSPLIT = 13,       // nodes to split at the next level
  SM_NTILES = 14,       // tiles of the next level
  SM_ETOTAL = 15,       // total of the scanned tile histogram
  SM_NBLOCKS = 16,      // blocks of the block table a build or an incremental insertion forms
  SM_BK_TICKET = 17,    // bucket build: workgroups of k_bucket_scan_totals that have finished (the last one forms the totals)
  SM_BK_OVERFULL = 18,  // bucket build: buckets with more than 4096 points (they are built in chunks of whole voxels)
  SM_SLOT_VOXELS = 21,  // octl_forest_get_slot_voxels: scan total = voxels in which the pose has points
  SM_BK_NOORDER = 23,   // bucket build: some bucket has too many nodes / blocks for k_bucket_finish's own block order
  SM_DEBUG_TOTAL = 24,  // octl_debug_exclusive_scan: scan total
  SM_BK_FLAGS = 25,     // bucket build: some bucket / voxel does not fit (BF_* bits)
  SM_BK_TOTAL = 26,     // bucket build: grand total of the scanned bucket table
  SM_BK_TODO = 27,      // bucket build: voxels left as one leaf for the level loop of build.hip
  SM_BK_MISSING = 28,   // bucket build over a previous scheme: voxels of that scheme without points now
                        // (build.hip's prefix partition, k_top_tree: some node above depth pm does not split)
  SM_CK_COUNT = 29,     // bucket build: chunks of the buckets with more than 4096 points (k_bucket_plan)
  SM_INC_MISS = 28,     // incremental insertion: new points whose voxel the scheme does not know
  SM_INC_BAD = 29,      // incremental insertion: new points outside a cube that is split
  SM_INC_DEAD = 30,     // incremental insertion: new points that are not alive
  SM_INC_NEWVOX = 31,   // incremental insertion: distinct new voxels
  SM_SLOT_COUNTS = 28,  // octl_forest_slot_counts: two u64 (points, leaves of the pose), words 28..31
  SM_BUILD_WORDS = 32,  // (end of the words k_build_begin resets)
  SM_MASK_TOTAL = 33,   // apply_mask without the fused kernel: grand total of its scan (written before it is read)
  SM_BK_LEVEL = 40,     // bucket build: internal nodes per level (7 words)
  SM_GEOM = 64,         // bucket build: key geometry formed on the device (GeomDev, <= 192 bytes)
  SM_SLOT_HIST = 128,   // forest_reference_order: blocks per pose slot (up to 256 words)
  SM_ALLREDUCE = 512,   // route.hip: int64 allreduce buffer (up to 256 values, to the end of the block)
  SM_WORDS = 1024
};
static_assert(SM_ERR < SM_BUILD_WORDS && SM_BBOX + 6 <= SM_BUILD_WORDS && SM_NVOX < SM_BUILD_WORDS &&
                  SM_NSPLIT < SM_BUILD_WORDS && SM_NTILES < SM_BUILD_WORDS && SM_ETOTAL < SM_BUILD_WORDS &&
                  SM_NBLOCKS < SM_BUILD_WORDS && SM_BK_TICKET < SM_BUILD_WORDS && SM_BK_OVERFULL < SM_BUILD_WORDS &&
                  SM_SLOT_VOXELS < SM_BUILD_WORDS &&
                  SM_BK_NOORDER < SM_BUILD_WORDS && SM_DEBUG_TOTAL < SM_BUILD_WORDS && SM_BK_FLAGS < SM_BUILD_WORDS &&
                  SM_BK_TOTAL < SM_BUILD_WORDS && SM_BK_TODO < SM_BUILD_WORDS && SM_BK_MISSING < SM_BUILD_WORDS &&
                  SM_CK_COUNT < SM_BUILD_WORDS && SM_INC_NEWVOX < SM_BUILD_WORDS &&
                  SM_SLOT_COUNTS + 4 <= SM_BUILD_WORDS,
              "the words a build starts from zero lie among the words k_build_begin resets");
static_assert(SM_MASK_TOTAL >= SM_BUILD_WORDS && SM_MASK_TOTAL < SM_BK_LEVEL,
              "apply_mask may be in flight beside the next build's front: its word is none of the front's");
static_assert(SM_BUILD_WORDS <= SM_BK_LEVEL && SM_BK_LEVEL + 7 <= SM_GEOM && SM_GEOM + 192 / 4 <= SM_SLOT_HIST &&
                  SM_SLOT_HIST + 256 <= SM_ALLREDUCE && SM_ALLREDUCE + 2 * 256 <= SM_WORDS,
              "scalar block regions");
uint32_t octl_wait_next_seq(octl_ctx* ctx);
int octl_wait_mirror_flags(octl_ctx* ctx, const int* words, int n_words, uint32_t seq, int64_t budget_us);
// device side: publish `seq` behind everything this thread (and, through the barriers in front of the call, its
// workgroup) has written to the mirror
__device__ __forceinline__ void mirror_publish(uint32_t* mirror, int word, uint32_t seq) {
  __threadfence_system();
  __hip_atomic_store(&mirror[word], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the compute stream waits (on the device, no host wait) for the uploads enqueued so far whose destination
// overlaps [p, p + bytes); p == nullptr: for all of them
int ctx_wait_uploads(octl_ctx* ctx, const void* p = nullptr, size_t bytes = 0);

#define HIP_TRY(ctx, expr)                                                                 \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return octl_set_error((ctx), OCTL_E_HIP, "%s failed: %s (%s:%d)", #expr,             \
                            hipGetErrorString(_e), __FILE__, __LINE__);                    \
  } while (0)

#define OCTL_TRY(expr)        \
  do {                        \
    int _r = (expr);          \
    if (_r != OCTL_OK) return _r; \
  } while (0)

// staging regions of ctx->pinned: wait until the previous asynchronous copy out of region r has
// finished / mark a new one as in flight
int pin_region_wait(octl_ctx* ctx, int r);
int pin_region_mark(octl_ctx* ctx, int r);
// copy `bytes` (a multiple of 8) from page-locked HOST memory to the device with a kernel on the context's
// stream: a small hipMemcpyAsync goes through the DMA queue and waits there behind a large upload that is in
// flight on the copy stream (measured: 2.9 ms per scan of the asynchronous feed)
// (`on`: the stream the copy goes to; nullptr = the context's)
int octl_copy_from_pinned(octl_ctx* ctx, void* dst_dev, const void* src_pinned, size_t bytes, hipStream_t on = nullptr);

// grow-only device buffer; contents are NOT preserved unless keep != 0
int devbuf_reserve(octl_ctx* ctx, DevBuf& b, size_t bytes, int keep = 0);
void devbuf_free(DevBuf& b);
// hand a block back to the context's pool (the stream must have finished with it) instead of freeing it
void devbuf_release(octl_ctx* ctx, DevBuf& b);

// RAII timer: records hipEvents around the launches in its scope when profiling is on
struct KTimer {
  octl_ctx* ctx;
  int idx = -1;
  KTimer(octl_ctx* c, const char* name);
  ~KTimer();
};
// fold the pending event pairs into ctx->timings (synchronises the stream)
int octl_collect_timings(octl_ctx* ctx);

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// byte offsets of the parts of a packed scratch buffer: every part starts 256-byte aligned
static inline constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// ... as a plan: add<T>(count) appends a part of `count` T behind the parts added so far, each rounded up by align256,
// and returns its typed handle; `total` is what devbuf_reserve is asked for, at(buffer, part) the part in a buffer that
// holds the plan from its first byte.
struct Carve {
  template <typename T>
  struct Part {
    size_t off = 0;
  };
  size_t total = 0;
  template <typename T>
  constexpr Part<T> add(size_t count) {
    const Part<T> part{total};
    total += align256(count * sizeof(T));
    return part;
  }
  template <typename T>
  static T* at(DevBuf& b, Part<T> part) {
    return reinterpret_cast<T*>(static_cast<char*>(b.p) + part.off);
  }
};
// workgroups of 256 threads for n items, one item per thread (n = 0: no workgroup - the caller guards or clamps)
static inline unsigned grid_for(int64_t n) { return (unsigned)ceil_div(n, 256); }
// bits needed to hold max_value (0 for 0)
static inline int bits_for(uint64_t max_value) {
  int b = 0;
  while (b < 64 && (max_value >> b) != 0) ++b;
  return b;
}
// blocking readback of `count` uint32 words from the device (the scalar block, as a rule) through the pinned mirror:
// one counted synchronisation of the context's stream
static inline int octl_readback(octl_ctx* ctx, const void* src_dev, int64_t count, void* out) {
  HIP_TRY(ctx, hipMemcpyAsync(ctx->small_host, src_dev, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(out, ctx->small_host, (size_t)count * 4);
  return OCTL_OK;
}

// the download of the first `count` elements of a part of a device table into `dst`, enqueued when the caller asked
// for that array (dst != nullptr) and it is not empty; *any = something is on its way: the caller waits once
template <typename T>
static inline hipError_t octl_download(octl_ctx* ctx, T* dst, DevBuf& src, Carve::Part<T> part, size_t count,
                                       bool* any) {
  if (!dst || count == 0) return hipSuccess;
  *any = true;
  return hipMemcpyAsync(dst, Carve::at(src, part), count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
}

// ---- device-wide primitives (scan.hip, radix_sort.hip) ------------------------------------
// exclusive prefix sum of n uint32 (in may equal out); if total_dev != nullptr the grand total
// (uint32) is written there.  n up to 2^31.
// compute units of the context's device (cached)
int octl_ctx_cus(octl_ctx* ctx);
// workgroups of 256 threads for n items taken grid-stride, one item per lane and pass: grid_for(n), at least one and at
// most 16 per compute unit
static inline unsigned grid_stride_for(octl_ctx* ctx, int64_t n) {
  const int64_t most = (int64_t)octl_ctx_cus(ctx) * 16, all = ceil_div(n, 256), wgs = all < most ? all : most;
  return (unsigned)(wgs > 1 ? wgs : 1);
}
// the side stream and its two events, created on first use; false when they cannot be had (not an error: the
// caller uses the context's stream)
bool octl_ctx_side_stream(octl_ctx* ctx);
int octl_exclusive_scan_u32(octl_ctx* ctx, const uint32_t* in, uint32_t* out, int64_t n,
                            uint32_t* total_dev);
// ---- the ahead stream (ctx.hip) ---------------------------------------------------------------------
// Points from which a build may run ahead when OCTL_BUILD_AHEAD_MIN_POINTS is not set.  No crossover was found: forced
// on, the 100 k-point scan of bench.py (secondary.small_scan_100k) is 0.117-0.123 ms against the parent's 0.124-0.125 with
// one cloud and 0.120-0.122 against 0.129-0.130 with three in turn (three repetitions each, interleaved, one box).  Nothing
// smaller was measured, so the bound is the smallest size that was.
constexpr int64_t OCTL_AHEAD_MIN_POINTS = 100000;
constexpr int64_t OCTL_AHEAD_TILES = 4096;  // status words of the ahead stream's look-back chain
static inline int64_t octl_ahead_min_points(const octl_ctx* ctx) {
  return ctx->opt.build_ahead_min_points >= 0 ? ctx->opt.build_ahead_min_points : OCTL_AHEAD_MIN_POINTS;
}
// the ahead stream, its two events and its status words, created on first use; false when they cannot be had (not an
// error: the build stays serial)
bool octl_ctx_ahead_stream(octl_ctx* ctx);
// Since the context's last build, did the library enqueue work under an AheadAllow on it, and nothing else?
bool octl_ahead_untouched(const octl_ctx* ctx, const struct octl_forest* f);
// Opens a front: the ahead stream waits for ahead_free and for the uploads still in flight into [cloud, cloud + bytes).
// false: nothing was enqueued there, the build is serial.
bool octl_ahead_open(octl_ctx* ctx, const void* cloud, size_t bytes);
// the stream a build's front goes to: the ahead stream while a front is open, else the context's
static inline hipStream_t octl_front_stream(const octl_ctx* ctx) { return ctx->ahead_open ? ctx->ahead_stream : ctx->stream; }
// The join: the context's stream waits for everything on the ahead stream.  No-op when no front is open.
void octl_ahead_join(octl_ctx* ctx);
// the end of a build of f: ok - the tally starts; else the context's next build is serial
void octl_ahead_build_end(octl_ctx* ctx, const struct octl_forest* f, bool ok, int64_t n_points);
// the first allow-listed function behind a build records ahead_free, if nothing else was enqueued in between
void octl_ahead_arm(octl_ctx* ctx);
// status words + a fresh epoch for a look-back chain ON THE AHEAD STREAM of up to OCTL_AHEAD_TILES workgroups
int octl_ahead_status_acquire(octl_ctx* ctx, int64_t tiles, uint64_t** status, uint32_t* epoch);
// Scope of a function whose device work touches nothing a build's front reads or writes (DESIGN 4.4.1 lists them with
// the reasons): what it enqueues is added to the context's tally, so that the next build may still run ahead.
// Scopes may nest (an allow-listed function that calls another one): only the outermost scope counts, so that nothing
// is added twice - a tally that is too large could balance an enqueue the list does not cover.
struct AheadAllow {
  octl_ctx* ctx;
  uint64_t at = 0;
  explicit AheadAllow(octl_ctx* c) : ctx(c) {
    if (ctx->ahead_allow_depth++ != 0) return;
    if (ctx->ahead_mark_pending) octl_ahead_arm(ctx);
    at = g_octl_enqueues.load(std::memory_order_relaxed);
  }
  ~AheadAllow() {
    if (--ctx->ahead_allow_depth == 0) ctx->ahead_allowed += g_octl_enqueues.load(std::memory_order_relaxed) - at;
  }
  AheadAllow(const AheadAllow&) = delete;
  AheadAllow& operator=(const AheadAllow&) = delete;
};
// status words + a fresh epoch for one look-back chain of up to `tiles` workgroups (lookback.h)
int octl_scan_status_acquire(octl_ctx* ctx, int64_t tiles, uint64_t** status, uint32_t* epoch);
// the allocations of a following octl_scan_status_acquire(tiles) / octl_exclusive_scan_u32(n) made now, so that neither
// can fail for memory (a transaction reserves before it changes anything)
int octl_scan_status_reserve(octl_ctx* ctx, int64_t tiles);
int octl_exclusive_scan_reserve(octl_ctx* ctx, int64_t n);
// stable LSD radix sort of (key u64, value u32) pairs on bits [0, key_bits).  keys[0]/vals[0]
// hold the input; keys[1]/vals[1] are ping-pong space of the same size.  *result (0 or 1)
// tells which pair of buffers holds the sorted output.
int octl_radix_sort_u64_u32(octl_ctx* ctx, uint64_t* keys[2], uint32_t* vals[2], int64_t n,
                            int key_bits, DevBuf& hist_scratch, int* result);
