// Declarations shared by the two build paths (build.hip: level-synchronous general path,
// bucket_build.hip: one MSD partition + one workgroup per bucket of voxels).
#pragma once
#include "forest.h"

constexpr uint32_t IDX_MASK = 0x7FFFFFFFu;

struct NodePtrs {
  uint32_t *start, *count, *scount;
  int32_t *depth, *voxel, *parent, *first_child, *old_id, *epoch;
  double *corner, *edge;
};

static inline NodePtrs node_ptrs(NodeTable& t) {
  NodePtrs p;
  p.start = t.start.as<uint32_t>();
  p.count = t.count.as<uint32_t>();
  p.scount = t.scount.as<uint32_t>();
  p.depth = t.depth.as<int32_t>();
  p.voxel = t.voxel.as<int32_t>();
  p.parent = t.parent.as<int32_t>();
  p.first_child = t.first_child.as<int32_t>();
  p.old_id = t.old_id.as<int32_t>();
  p.epoch = t.epoch.as<int32_t>();
  p.corner = t.corner.as<double>();
  p.edge = t.edge.as<double>();
  return p;
}

// bucket_build.hip: complete build of a fresh forest (K-driven scheme or K < 0, no previous scheme) by
// one MSD partition into buckets of consecutive voxels + one workgroup per bucket (BucketBuildResult::done
// = 0 when the path does not apply and the caller must run the general path).
struct BucketBuildArgs {
  int64_t K;
  const uint8_t* scheme_dev;  // per pose slot: 1 = the pose drives the scheme; nullptr = all poses
  int cur_epoch;
  int max_depth;
  // the previous scheme (subdivide on an already subdivided forest): nodes that were internal before keep
  // their epoch, and every voxel of the previous scheme has to be there again.  nullptr / 0 when fresh.
  const int32_t* old_fc = nullptr;
  const int32_t* old_epoch = nullptr;
  const uint64_t* old_vcode = nullptr;  // sorted packed voxel keys; old root r = voxel r
  int64_t old_voxels = 0;
};
struct BucketBuildGeom {  // decoding of the linear voxel keys: lin = ((qx-min0)*ny + (qy-min1))*nz + (qz-min2)
  int min[3];
  uint64_t ny, nz;
  bool order_done = false;  // f->fast_order holds the blocks in the reference's listing order
};
struct BucketBuildResult {
  int done = 0;  // 1: the build is complete; 0: the path does not apply, the caller runs the general one
  std::vector<octl_forest::LevelSeg> segs;
  int64_t n_internal = 0;
  int levels = 0;
  int64_t n_voxels = 0, n_blocks = 0;
  int64_t pending = 0;  // voxels left as single leaves for the level loop of build.hip (flagged roots)
  BucketBuildGeom geom;
};
int forest_bucket_build(octl_forest* f, const BucketBuildArgs& a, NodeTable& nt, BucketBuildResult* r);
// Will the first attempt of forest_bucket_build(f) be ONE partition pass under the context's hint, over a cloud taken in
// place with every point alive, with its tables scanned by k_table_scan / the scatter kernel itself, and without
// growing a buffer that pass writes (part_xyz[0], bk_table)?  Host arithmetic, no side effect: what forest_build asks
// before it puts the front on the ahead stream.  (A wrong "yes" costs nothing but the overlap: partition() joins
// the streams in front of whatever it did not expect.)
bool forest_bucket_front_fits(const octl_forest* f);

// bucket_build.hip: one stable partition of a single cube's store by the child digits of its first pm levels
// (records of 32 bytes: x, y, z f64 | six digits << 1 | bad | store index + scheme bit).  The layout as the readers
// of the records in build.hip use it (general_level0: k_pre_level0, general_level_loop, general_finalize:
// k_finalize_rec); bucket_build.hip ties it to PartRec and PATH_EAGER.
constexpr int PART_REC_BYTES = 32;
constexpr int PART_REC_QUADS = PART_REC_BYTES / 16;      // 16-byte accesses per record
constexpr int PART_REC_DOUBLES = PART_REC_BYTES / 8;     // stride of the coordinates, in doubles (LevelLoop::xs)
constexpr int PART_REC_VP_WORD = 6;                      // 32-bit word that holds vp ...
constexpr int PART_REC_IDX_WORD = 7;                     // ... and the one that holds the store index
constexpr int PART_VP_DIGITS = 6;                        // child digits vp carries, first level highest
constexpr int PART_VP_DIGIT_BITS = 3 * PART_VP_DIGITS;
constexpr int PART_VP_DIGIT_SHIFT = 1;
constexpr uint32_t PART_VP_DIGIT_MASK = (1u << PART_VP_DIGIT_BITS) - 1u;
constexpr uint32_t PART_VP_BAD = 1u;                     // the point is outside the cube at some level
int forest_prefix_partition(octl_forest* f, int pm, const void** recs_out, const uint32_t** bstart, uint32_t* bstride,
                            const uint32_t** bad_flag);
