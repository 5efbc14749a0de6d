// Device-resident state of one Grid / OctreeManager / Octree ("forest" of top-level cubes).
#pragma once
#include "common.h"

// packed voxel key: (qx-ox+B)<<42 | (qy-oy+B)<<21 | (qz-oz+B), B = 2^20; lexicographic (x,y,z) order of
// the integer voxel coordinates == numeric order of the key (np.unique(axis=0) order,
// grid/grid.py:79-81).  The key is RELATIVE to the forest's voxel origin o - the minimum voxel of the first
// build after a clear (forest_fix_origin) - so that voxel indices of any size work (the reference takes any
// int64, grid.py:72-76: UTM coordinates at 1 m voxels are 5 * 10^6) as long as the scene stays within 2^20
// voxels of where it started; absolute indices are limited to +-2^30 (they travel as int32).
#define OCTL_VOX_BIAS (1 << 20)
#define OCTL_VOX_ABS_LIMIT (1 << 30)
#define OCTL_VOX_DEAD (~0ull)
struct VoxOrg {
  int32_t x = 0, y = 0, z = 0;
};
__host__ __device__ static inline uint64_t vkey_pack(int64_t qx, int64_t qy, int64_t qz, const VoxOrg& g) {
  return ((uint64_t)(qx - g.x + OCTL_VOX_BIAS) << 42) | ((uint64_t)(qy - g.y + OCTL_VOX_BIAS) << 21) |
         (uint64_t)(qz - g.z + OCTL_VOX_BIAS);
}
__host__ __device__ static inline bool vkey_in_window(int64_t qx, int64_t qy, int64_t qz, const VoxOrg& g) {
  const int64_t ax = qx - g.x, ay = qy - g.y, az = qz - g.z;
  return ax > -OCTL_VOX_BIAS && ax < OCTL_VOX_BIAS && ay > -OCTL_VOX_BIAS && ay < OCTL_VOX_BIAS &&
         az > -OCTL_VOX_BIAS && az < OCTL_VOX_BIAS;
}
__host__ __device__ static inline void vkey_decode(uint64_t k, const VoxOrg& g, int64_t q[3]) {
  q[0] = (int64_t)((k >> 42) & 0x1FFFFF) - OCTL_VOX_BIAS + g.x;
  q[1] = (int64_t)((k >> 21) & 0x1FFFFF) - OCTL_VOX_BIAS + g.y;
  q[2] = (int64_t)(k & 0x1FFFFF) - OCTL_VOX_BIAS + g.z;
}

// Structure-of-arrays scheme node table on the device.
struct NodeTable {
  DevBuf start, count, scount;  // u32: range in the level buffers, scheme-pose point count
  DevBuf depth, voxel, parent, first_child, old_id, epoch;  // i32
  DevBuf corner, edge;          // f64 x3, f64
  int64_t cap = 0, n = 0;
};

// the second split rule of octl_forest_build_planar (criteria.py: NotPlanar): a node with at least min_points scheme
// points splits when the smallest eigenvalue of their covariance (divisor n - ddof) exceeds max_variance
struct PlanarRule {
  double max_variance;
  int32_t min_points, ddof;
};

struct octl_forest {
  octl_ctx* ctx = nullptr;
  int mode = 0;  // 0 grid, 1 single cube
  double corner[3] = {0, 0, 0};
  double edge = 1.0;

  // point store: all poses concatenated in slot order (pose-major), insertion order inside
  DevBuf xyz;     // f64 [n_store][3]
  DevBuf alive;   // u8  [n_store]
  DevBuf alive2;  // octl_forest_remove_poses: the flags of the squeezed store are written here, then the two swap
  // octl_forest_add_pose_adopt: xyz.p is the CALLER's device buffer (read in place, never written, never
  // freed here); the forest's own block waits in xyz_own and the store is copied into it (store_materialize)
  // before anything appends to or reorders the store
  bool store_borrowed = false;
  DevBuf xyz_own;
  // the store's points have not been folded into bbox_dev yet (a cloud taken in place: adopted or routed).
  // Only ever set while the store is that ONE pose; the build folds the box into its histogram pass when it
  // has a geometry hint to work with, or runs the box pass first (store_compute_bbox)
  bool bbox_pending = false;
  // octl_forest_set_contents left rows OUTSIDE the cube of the leaf that holds them (map_leaf_points may return
  // anything, octree.py:114-123).  The reference keeps such rows in that leaf and raises IndexError as soon as the
  // leaf is split; a count-driven build here would silently re-bucket them by their coordinates - so it refuses.
  bool displaced_rows = false;
  std::vector<int64_t> pose_off{0};  // [P+1] offsets into the store
  int64_t n_store = 0, n_alive = 0;
  bool store_dirty = true;  // points were added/removed since the last build
  // what the last build covered, for the incremental insertion of incremental.hip: the store prefix
  // and the poses the tables describe, and whether every change since was a pose appended behind them
  int64_t built_store = 0;
  int built_poses = 0;
  bool append_only = true;
  // voxel bounding box of every point added since the last clear, kept by the ingest kernel
  // (store.hip): int32 x 8 = {min x,y,z, max x,y,z, domain-error flag, point outside a hinted box}
  DevBuf bbox_dev;
  // octl_forest_clear does not launch anything: the box on the device is STALE until something resets it - the next
  // ingest / box pass (bbox_ensure), or the first kernel of a build that finds the box itself (k_build_begin)
  bool bbox_stale = true;
  // the alive flags of a cloud taken in place (adopted, routed) are not written until something needs them
  // (alive_ensure: a second pose, a re-placement; apply_mask fills them in its first kernel): every point is alive
  bool alive_stale = false;
  // octl_forest_transform_poses (store.hip): the table one call uploads - the fresh box, the poses' end offsets, a
  // 3x4 and a selected flag per pose; octl_forest_remove_poses: its table (RetireLayout)
  DevBuf xf_tab;

  // scheme of the last build
  NodeTable nodes[2];
  int cur = 0;               // nodes[cur] is the current table
  int epoch = 0;             // number of K-driven builds so far
  bool built = false;
  VoxOrg vorg;                  // voxel origin of the packed keys (fixed by the first build after a clear)
  bool vorg_set = false;
  std::vector<uint64_t> vkeys;  // packed integer coordinates of the top-level voxels, sorted
                                // (filled lazily from vlin_dev: forest_sync_vkeys)
  bool vkeys_stale = false;
  int64_t n_voxels = 0;
  DevBuf vcode_dev[2];          // u64 [n_voxels] sorted packed voxel keys on the device (forest_sync_vcodes); [1] = scratch
  bool vcode_valid = false;
  DevBuf vlin_dev;              // u64 [n_voxels] compact linear voxel keys of the last build
  int vl_min[3] = {0, 0, 0};    // decoding of vlin_dev: lin = ((qx-min0)*ny + (qy-min1))*nz + (qz-min2)
  uint64_t vl_ny = 1, vl_nz = 1;
  int64_t n_internal = 0;
  bool uniform_epoch = true;  // every internal node of the current scheme has the same epoch
  int32_t max_depth_reached = 0;
  // octl_forest_get_split_stats: what the split decisions of the last planar build saw, per node of the current
  // table - the statistic (split_planar.hip writes it level by level) and the scheme-point count (copied when the
  // build commits).  Valid while the table is the one that build left: any later build that renumbers it drops them.
  DevBuf split_lambda, split_n;  // f64, u32 [split_stats_nodes]
  bool split_stats_valid = false;
  int64_t split_stats_nodes = 0;

  // ---- derived map tables: made from the block table, the ordered points, the node table and the pose offsets, and
  // kept until one of those changes.  Whoever changes one calls forest_contents_changed (below), which moves
  // content_stamp on.  A table records the stamp it was made at in X_stamp - 0: none; zeroed when its prepare / compute
  // function starts, set when it has succeeded, so one that failed half way stays invalid - and is valid while that is
  // the forest's (forest_table_valid).  Each keeps the pose selection it was made for too (X_sel, empty: every pose):
  // another selection makes it again.  The packed tables are Carve plans (common.h).
  uint64_t content_stamp = 1;
  // what the pooled planes, the adjustment tables and the neighbour index need while they are made and nobody reads
  // once that function has returned - the (node, slot) grouping of the blocks (leaf_moments.h: block_groups) with the
  // function's own words behind it - and the histograms of every radix sort.  One stream per forest: one of each.
  // (The three layouts differ by a few hundred bytes, which the slack of devbuf_reserve takes as a rule; where it does
  // not, the first call of one behind another grows a buffer in use, which costs that call one host wait.)
  DevBuf grp_scratch, pl_hist;

  // octl_forest_pooled_leaf_stats (leaf_stats.hip): one plane per leaf over a selection of poses.  pl_rows holds the
  // result table of the last call as it is downloaded (PoolLayout below, for pl_cap rows), pl_plane the 64-byte rows
  // octl_forest_point_to_plane gathers {nx, ny, nz, mx, my, mz, lambda0, (double)count}, pl_node_row the row of every
  // scheme node (-1: none; allocated by the first computation, which is how query_plane_table tells "none" from
  // "stale").
  DevBuf pl_rows, pl_plane, pl_node_row;
  uint64_t pl_stamp = 0;
  int64_t pl_n = 0, pl_cap = 0;
  std::vector<uint8_t> pl_sel;
  DevBuf q_stage;               // staging of the host forms of the queries (points in, answers out)
  DevBuf rg_rows;               // the three registration systems (reg_driver.h: reg_scratch): result, rows, records

  // octl_forest_adjustment_system (adjust.hip), prepared once per map and pose selection:
  //  adj_tab   the selected (leaf, pose) blocks in (node, slot) order - 80-byte moments {n, sum d, sum d d^T} about the
  //            leaf's centre, leaf row and selection index of every block - the leaves (first block, node, anchor), the
  //            second order of the same blocks by (slot, node) and its chunks of at most 1024 blocks of one pose;
  //  adj_call  what one call writes: transforms, the plane row of every leaf, the per-chunk partial sums, the result.
  DevBuf adj_tab, adj_call;
  uint64_t adj_stamp = 0;
  bool adj_called = false;           // adj_call holds the leaf table of a call on this preparation
  std::vector<uint8_t> adj_sel;
  std::vector<int32_t> adj_slots;    // slot of every selected pose, ascending
  std::vector<int64_t> adj_chunk_off;  // [S + 1] first chunk of every selected pose
  int64_t adj_blocks = 0, adj_rows = 0;  // selected blocks, leaves that hold one

  // octl_forest_nearest (nearest.hip): the index node -> run of selected (leaf, pose) blocks in slot order, made by
  // the call that finds none that is valid.  nn_tab: one 16-byte record {start, size, slot, store offset of the pose}
  // per block in (node, slot) order, then first record and number of records of every node of the scheme.
  DevBuf nn_tab;
  uint64_t nn_stamp = 0;
  std::vector<uint8_t> nn_sel;

  // octl_forest_plane_segments (segments.hip): the face adjacency of the rows of the pooled table, the connected
  // components of the coplanar ones and one merged plane per component, cached with the arguments they were made for.
  // A pooled table made again for another selection drops them too (octl_forest_plane_segments zeroes seg_stamp).
  // seg_sort is the scratch of one computation (union-find, head flags, sort, segment starts).  It is not grp_scratch:
  // sized by the rows, and a first call would grow that buffer while the pooled table's kernels read it - a host wait.
  DevBuf seg_tab, seg_out, seg_sort;  // (SegRowLayout, SegOutLayout: segments.hip)
  uint64_t seg_stamp = 0;
  int64_t seg_rows = 0, seg_n = 0, seg_cap = 0;  // rows the tables were made for, segments, segments the layout holds
  std::vector<uint8_t> seg_sel;
  int32_t seg_min_points = 0;
  double seg_max_variance = -1.0, seg_cos_min = 0.0, seg_max_offset = 0.0;

  // leaf-ordered arrays of the last build
  DevBuf ord_idx;    // u32 [n_ord] store index of the point at storage position i
  DevBuf xyz_ord;    // f64 [n_ord][3]
  DevBuf pos_node;   // i32 build scratch: scheme leaf of position i while a build runs (afterwards the block
                     // table alone says which leaf a position belongs to)
  int64_t n_ord = 0;
  // non-empty (leaf, pose) blocks in storage order
  DevBuf blk_node, blk_slot, blk_start, blk_size;  // i32, i32, u32, i32
  int64_t n_blocks = 0;
  // RANSAC state
  DevBuf mask;       // u8 [n_ord]
  DevBuf blk_eval;   // u8 [n_blocks] block was evaluated since the last apply_mask
  bool mask_valid = false;
  // octl_forest_apply_mask_async: the kernels are enqueued and the arrays swapped, the surviving point / block counts
  // are still on their way to the pinned mirror - forest_settle (every entry point's first step) waits for them
  bool totals_pending = false;
  uint32_t totals_seq = 0;      // wait sequence number the kernels publish under
  int64_t totals_n_before = 0;  // ordered points before the compaction

  // an upper bound of the points a block can hold, when the host knows one (a count-driven build from all poses
  // leaves at most K points per leaf, and masks / filters only remove points): the RANSAC launch skips the instances
  // for block sizes that cannot occur.  INT64_MAX: unknown (late poses, installed schemes, replaced contents ...)
  int64_t max_block_hint = INT64_MAX;
  DevBuf rs_scratch, rs_order, rs_hyp, rs_plane, rs_count, rs_index;  // ransac staging
  // the blocks in the reference's listing order as the bucket build left them (one pose, one epoch):
  // forest_reference_order takes this instead of computing it; any change of the blocks invalidates it
  DevBuf fast_order;
  bool fast_order_valid = false;
  // what pose_off_dev holds (offsets that have not changed are not uploaded again)
  std::vector<int64_t> pose_off_uploaded;
  DevBuf ord_idx2, xyz_ord2;  // compaction targets (swapped with the live arrays)
  DevBuf blk_node2, blk_slot2, blk_start2, blk_size2;

  // bucket build (bucket_build.hip): the cloud partitioned into buckets of consecutive voxels
  DevBuf part_xyz[2];  // 32-byte records {x, y, z, voxel | child digits, store index | scheme bit}, two passes
  DevBuf bk_table;     // u32 [digit][supertile] partition histogram (scanned in place)
  DevBuf bk_tot;       // u32 [BK_ROWS][n_buckets] per-bucket totals (scanned in place)
  DevBuf bk_chunks;    // chunk plan of the buckets with more than 4096 points: descriptors, per-chunk totals, range per bucket
  DevBuf bk_vox;       // u32 x3 staging {linear key, points | todo, scheme points} of the j-th voxel of bucket b
                       // at [bucket start + j]
  DevBuf bk_node;      // u32 x3 staging {voxel << 18 | path, level << 28 | ordinal, parent ordinal} of the j-th internal
                       // node of bucket b at [bucket start + j]
  DevBuf leafinfo;     // u32 [n_alive] per leaf-ordered point: leaf in bucket terms (parent ordinal, child digit, depth) | head flags
  // levels of the current node table as (first, end, depth) ranges of node ids: one per level when a
  // single build path numbered the nodes, two where the level loop has subdivided voxels the bucket
  // build left behind (order.hip sweeps them by depth)
  struct LevelSeg { int64_t a, b; int depth; };
  std::vector<LevelSeg> level_segs;
  // build scratch (kept between builds to avoid re-allocation)
  DevBuf vkey, path, lin[2], val[2], hist, idxbuf[2], pathbuf[2], flags, entries, split[2],
      split_tiles[2], child_sc, pose_off_dev, scheme_dev, root_up;
};

// planar != nullptr: the scheme for "count > K OR planar rule" (K < 0: no count rule), always through the level loop
int forest_build(octl_forest* f, int64_t K, const uint8_t* scheme_mask, int32_t n_mask,
                 int32_t keep_scheme, int32_t max_depth, octl_build_info* info, const PlanarRule* planar = nullptr);
// split_planar.hip: the planar statistic of the fresh nodes [first_new, first_new + n_new) of table nt into
// f->split_lambda; idx = the level buffer that holds their points, xyz / xs = the coordinates behind its indices
int planar_level_stats(octl_forest* f, const PlanarRule& rule, NodeTable& nt, int64_t first_new, int64_t n_new,
                       const uint32_t* idx, const double* xyz, int xs, int64_t n_alive);
int nodes_reserve(octl_ctx* ctx, NodeTable& t, int64_t cap);
void nodes_free(octl_ctx* ctx, NodeTable& t);

// ransac.hip
int ransac_launch(octl_ctx* ctx, const double* xyz_dev, int64_t n_points,
                  const uint32_t* blk_start, const int32_t* blk_size, const int32_t* order_dev,
                  int64_t nb, const double* hyp_dev, int32_t H, int32_t k, double thr,
                  uint8_t* mask_dev, float* plane_dev, int32_t* count_dev, int32_t* index_dev,
                  uint8_t* evaluated_dev, DevBuf& scratch, int64_t max_block = INT64_MAX);
// the hypothesis table must hold draws from [0, 1) (np.random.random, cuda_ransac.py:39-41): anything
// else would index outside the block in the sampling arithmetic (cuda_ransac.py:103-107)
int ransac_check_table(octl_ctx* ctx, const double* hyp, int32_t H, int32_t k);
// store.hip: an empty store takes over a library-owned device buffer (swap) instead of copying it
int store_adopt(octl_forest* f, DevBuf& src, int64_t n, bool* adopted);
// store.hip: fold the whole store into bbox_dev (clears bbox_pending); copy a borrowed store into the forest's own block
int store_compute_bbox(octl_forest* f);
int store_materialize(octl_forest* f);
// store.hip: the box on the device is valid (reset if octl_forest_clear left it stale) / the alive flags are written
int bbox_ensure(octl_forest* f);
int alive_ensure(octl_forest* f);
// build.hip: (re)build the (leaf, pose) block table from pos_node / ord_idx
int forest_make_blocks(octl_forest* f);
// reads the block count (and the domain-error flag) left on the device: one synchronisation
int forest_finish_blocks(octl_forest* f, uint32_t* err_out);
// host copy of the voxel keys (synchronises when stale)
int forest_sync_vkeys(octl_forest* f);
// build.hip: fix the voxel origin of the packed keys from a voxel box (first build after a clear) and check
// that the box lies inside the window of the keys; OCTL_E_DOMAIN otherwise
int forest_fix_origin(octl_forest* f, const int bb[6]);
// incremental.hip: device copy of the packed voxel keys; poses appended to a built forest placed into
// its scheme in O(new points).  *done = 0: not applicable, nothing was changed.  wait = false: an upload of the host's
// keys is not waited for - the caller waits for the stream before f->vkeys can change
int forest_sync_vcodes(octl_forest* f, bool wait = true);
int forest_insert_incremental(octl_forest* f, int* done, octl_build_info* info);

// The block table, the ordered points, the node table or the pose offsets have changed or are about to (a pose added
// or extended, a build, a scheme or contents installed, points masked or filtered away, a clear, a scheme dropped):
// every derived map table of the forest is stale from here on.
static inline void forest_contents_changed(octl_forest* f) { ++f->content_stamp; }
// api.hip: the forest forgets its scheme, its voxels and every table made from them - what octl_forest_clear leaves,
// whatever the store holds (octl_forest_clear empties it first; octl_forest_transform_poses has just moved its rows)
void forest_reset_scheme(octl_forest* f);
// the table that recorded `stamp` describes the forest as it is now
static inline bool forest_table_valid(const octl_forest* f, uint64_t stamp) { return stamp == f->content_stamp; }
// the pose selection of a map query as the tables keep it (empty: every pose); one entry per pose or refused
static inline int forest_selection(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, std::vector<uint8_t>* sel) {
  const int n_poses = (int)f->pose_off.size() - 1;
  if (slot_sel && n_sel != n_poses)
    return octl_set_error(f->ctx, OCTL_E_INVALID, "slot selection has %d entries for %d poses", n_sel, n_poses);
  sel->assign(slot_sel, slot_sel + (slot_sel ? n_poses : 0));
  return OCTL_OK;
}

// leaf_stats.hip: layout of f->pl_rows for `cap` rows, and the pooled table of the selection `sel` (empty: every pose)
// of the forest as it stands - what octl_forest_pooled_leaf_stats and octl_forest_plane_segments make when they find
// none that is valid
struct PoolLayout {
  size_t c;  // rows (at least one)
  Carve plan;
  Carve::Part<int32_t> node = plan.add<int32_t>(c);
  Carve::Part<int64_t> count = plan.add<int64_t>(c);
  Carve::Part<double> mean = plan.add<double>(3 * c), cov = plan.add<double>(6 * c), w = plan.add<double>(3 * c),
                      v = plan.add<double>(9 * c);
  constexpr explicit PoolLayout(int64_t cap) : c((size_t)(cap > 1 ? cap : 1)) {}
};
static_assert(PoolLayout(100).cov.off == 4096 && PoolLayout(100).v.off == 11520 && PoolLayout(100).plan.total == 18944,
              "PoolLayout offsets: a part starts where the 256-byte-rounded parts before it end");
int pooled_compute(octl_forest* f, const std::vector<uint8_t>& sel);

// mask.hip: wait for the counts an asynchronous apply_mask left in flight (octl_forest_apply_mask_async) and book
// them; a no-op otherwise.  Every entry point that looks at the forest calls it first.
int forest_settle(octl_forest* f);
// ... and forget them (clear / destroy: nothing will look at the counts)
void forest_forget_pending(octl_forest* f);
// mask.hip: the RANSAC mask is allocated and, when it is not valid, all ones (every point kept)
int ensure_mask(octl_forest* f);
// mask.hip, for octl_forest_remove_poses (store.hip, store_retire.h).  mask_retire_reserve: every buffer the two calls
// below grow, grown - nothing the forest reads has changed when it fails.  mask_retire_slots: the blocks of the poses
// with sel_dev[slot] != 0 are cleared in the mask (a pending RANSAC mask stays in it; without one every other byte
// becomes 1), their sizes are added to *removed_dev, and the ONE compaction runs (the host waits for its counts).
int mask_retire_reserve(octl_forest* f);
int mask_retire_slots(octl_forest* f, const uint8_t* sel_dev, unsigned long long* removed_dev);
// mask.hip, for octl_forest_remove_sparse (radius.hip): the ONE compaction over f->mask as it stands (valid: the
// caller has cleared its bytes in it, a pending RANSAC mask with them); *n_alive (nullable) = points left
int mask_apply(octl_forest* f, int64_t* n_alive);
