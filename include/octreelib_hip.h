/*
 * octreelib_hip.h — C ABI of liboctree_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for octreelib's point-cloud -> octree-grid build-and-query
 * path.  The reference (prime-slam/octreelib, /root/reference) has no FFI of its own: its
 * boundary is the Python class surface plus ONE device operator.  Every entry point below
 * names the reference interface it replaces (paths relative to /root/reference):
 *
 *   octl_forest_*            Grid / OctreeManager / Octree state
 *                            grid/grid.py:49-56, octree_manager/octree_manager.py:21-34,
 *                            octree/octree_base.py:143-158
 *   octl_forest_add_pose     Grid.insert_points                grid/grid.py:58-109
 *                            OctreeManager.insert_points       octree_manager.py:161-171
 *                            Octree.insert_points              octree/octree.py:235-239
 *   octl_forest_build        Grid.subdivide                    grid/grid.py:244-258
 *                            OctreeManager.subdivide           octree_manager.py:36-66
 *                            OctreeNode.subdivide/_as          octree/octree.py:20-53
 *                            OctreeNode.insert_points          octree/octree.py:67-100
 *                            OctreeNode._generate_children     octree/octree.py:177-191
 *   octl_forest_ransac       Grid.map_leaf_points_cuda_ransac  grid/grid.py:124-215
 *   octl_forest_apply_mask   OctreeManager/Octree.apply_mask   octree_manager.py:173-180,
 *                                                              octree/octree.py:265-274
 *   octl_ransac_evaluate     CudaRansac.evaluate               ransac/cuda_ransac.py:43-81
 *                            kernel                            ransac/cuda_ransac.py:85-155
 *                            get_plane_from_points             ransac/util.py:27-84
 *                            measure_distance                  ransac/util.py:12-24
 *
 * Conventions
 *   - every function returns 0 on success, a negative OCTL_E_* code on failure; the text of
 *     the last failure on a context is octl_last_error(ctx).  No exception crosses the ABI.
 *   - host buffers belong to the caller and are only touched during the call; all device
 *     memory belongs to the context / forest.  Calls are blocking with respect to host
 *     buffers.  A context is bound to one device and one HIP stream and is not thread safe
 *     (one context per GPU; multi-GPU = one process per rank).
 *   - "pose slot" = index of a pose in insertion order (0..P-1); the Python layer maps the
 *     user's pose numbers to slots.
 *   - coordinates are float64 row-major (n,3), exactly as the reference stores them
 *     (internal/voxel.py:81-83).
 */
#ifndef OCTREELIB_HIP_H
#define OCTREELIB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCTL_ABI_VERSION 1

enum {
  OCTL_OK = 0,
  OCTL_E_INVALID = -1,    /* bad argument                                              */
  OCTL_E_HIP = -2,        /* HIP runtime error (message has the hipError string)        */
  OCTL_E_NOMEM = -3,      /* device or host allocation failed                           */
  OCTL_E_DOMAIN = -4,     /* input outside the parity domain (point outside its cube,
                             non-finite coordinate, voxel index out of range)            */
  OCTL_E_DEPTH = -5,      /* max_depth exceeded (duplicate points with a count criterion
                             recurse forever in the reference)                           */
  OCTL_E_STATE = -6,      /* call out of order (e.g. ransac before build)               */
  OCTL_E_COMM = -7        /* RCCL error                                                  */
};

typedef struct octl_ctx octl_ctx;
typedef struct octl_forest octl_forest;

/* ---- context ------------------------------------------------------------------------ */
int octl_abi_version(void);
int octl_device_count(int* count);
int octl_ctx_create(int device_id, octl_ctx** out);
void octl_ctx_destroy(octl_ctx* ctx);
const char* octl_last_error(const octl_ctx* ctx);
/* synchronise the context's stream */
int octl_ctx_sync(octl_ctx* ctx);
/* timing of the kernels launched by the last build / ransac call, by name; fills up to cap
 * entries, returns the number available through *n.  Milliseconds from hipEvents on the
 * context's stream; only recorded when profiling was enabled with octl_ctx_set_profiling:
 * 1 = every timed region, 2 = the RANSAC scoring kernel only (every hipEvent pair drains the
 * pipeline for ~10 us: a dozen of them are 2 % of a 10 M-point step), 0 = off.               */
int octl_ctx_set_profiling(octl_ctx* ctx, int enabled);
int octl_ctx_get_timings(octl_ctx* ctx, char* names, int name_stride, float* ms,
                         int64_t* launches, int cap, int* n);

/* ---- forest: a Grid (many top-level voxels) or one cube (Octree / OctreeManager) ------ */

/* mode 0: grid of top-level voxels of edge L anchored at grid_corner (GridConfig.
 *         voxel_edge_length / corner, grid/grid_base.py:70-71).  L must be integer valued
 *         (the reference truncates voxel coordinates with astype(int), grid.py:72-76).
 * mode 1: a single cube [corner, corner+edge)^3 (Octree(config, corner_min, edge_length) /
 *         OctreeManager(..., corner_min, edge_length)).                                    */
int octl_forest_create(octl_ctx* ctx, int mode, const double corner[3], double edge,
                       octl_forest** out);
void octl_forest_destroy(octl_forest* f);

/* Forget all poses and the scheme but keep the device allocations (a fresh Grid without the
 * hipMalloc cost).                                                                          */
int octl_forest_clear(octl_forest* f);

/* Append the cloud of a new pose slot (host pointer, copied to the device).  Returns the
 * slot through *slot.  Replaces Grid.insert_points' storage step.                        */
int octl_forest_add_pose(octl_forest* f, const double* xyz, int64_t n, int32_t* slot);
/* Same, from a device pointer (device-to-device copy fused with the bounding-box pass; no PCIe).  The
 * source is consumed in stream order: it must stay unchanged until a call that leaves the context's stream IDLE:
 * octl_ctx_sync and every call that downloads to host memory (octl_forest_get_mask, _get_blocks, _get_nodes,
 * _gather_blocks, ...).  NOT among them since round 5: octl_forest_build and octl_forest_apply_mask - they
 * return when the scalars they hand back have arrived in the pinned mirror, while their last kernels may still
 * be running (stream order is kept: anything enqueued on the context afterwards runs behind them).           */
int octl_forest_add_pose_device(octl_forest* f, const double* xyz_dev, int64_t n,
                                int32_t* slot);
/* Same, WITHOUT the copy: an empty forest reads the caller's device buffer in place as its first pose
 * (Grid.insert_points' storage step, grid/grid.py:58-109, for a cloud that is in HBM already).  The library
 * never writes to the buffer and never frees it; the caller keeps it alive and unchanged until the forest is
 * cleared or destroyed, or until more points are added to it (octl_forest_add_pose*, octl_forest_extend_pose
 * take a private copy first).  A forest that already holds points, or a pointer that is not 16-byte aligned,
 * takes the copying path of octl_forest_add_pose_device.  The voxel bounding box of such a cloud is found by the
 * build's own histogram pass when the context has built a cloud of the same scene before, by a box pass
 * (24 B/point read) otherwise.                                                                    */
int octl_forest_add_pose_adopt(octl_forest* f, const double* xyz_dev, int64_t n, int32_t* slot);
/* Replace the CONTENTS of the leaves and keep the scheme: OctreeNode.map_leaf_points (octree/octree.py:114-123)
 * stores whatever the caller's function returned for a leaf's cloud - fewer rows, more rows, rows outside the
 * leaf's cube.  The new non-empty (leaf, pose) blocks are given in storage order: leaf node, pose slot, size, and
 * the rows of all blocks one after the other.  The point store is rebuilt (pose-major, a pose's points in the
 * order of its blocks); a later subdivide re-places the points by their coordinates (a row outside its cube then
 * fails where the reference raises IndexError).                                                          */
int octl_forest_set_contents(octl_forest* f, int64_t n_blocks, const int32_t* blk_node, const int32_t* blk_slot,
                             const int32_t* blk_size, const double* xyz);
/* Append more points to an EXISTING pose slot, any slot (OctreeManager.insert_points on a pose that
 * already has an octree, octree_manager.py:161-171; Octree.insert_points, octree.py:235-239).  The
 * points of later poses move up in the pose-major store.                                       */
int octl_forest_extend_pose(octl_forest* f, int32_t slot, const double* xyz, int64_t n);
/* Same, from a device pointer (device-to-device copy; ordered behind an octl_dev_upload_async into it).  */
int octl_forest_extend_pose_device(octl_forest* f, int32_t slot, const double* xyz_dev, int64_t n);

/* float32 clouds (row-major (n,3) float).  The reference upcasts every cloud to f64 before any arithmetic
 * (internal/voxel.py:81-83: np.vstack onto an f64 array; the grid's voxel corners are f64), and f32 -> f64 is exact:
 * each entry below leaves the forest exactly as its f64 counterpart leaves it for the widened cloud - store, tables,
 * counts, errors.  The widening runs on the device (12 B per point cross PCIe instead of 24); the store stays f64.  */
/* Grid.insert_points (grid/grid.py:58-109), OctreeManager.insert_points (octree_manager.py:161-171) and
 * Octree.insert_points (octree/octree.py:235-239) of an f32 host cloud: octl_forest_add_pose.  The host buffer is
 * the caller's again when the call returns.                                                                    */
int octl_forest_add_pose_f32(octl_forest* f, const float* xyz, int64_t n, int32_t* slot);
/* The same from a device pointer: octl_forest_add_pose_device (consumed in stream order, ordered behind an
 * octl_dev_upload_async into it).  Never read in place: the points are widened into the forest's own store.    */
int octl_forest_add_pose_device_f32(octl_forest* f, const float* xyz_dev, int64_t n, int32_t* slot);
/* OctreeManager.insert_points on an existing pose (octree_manager.py:161-171), Octree.insert_points
 * (octree/octree.py:235-239): octl_forest_extend_pose for an f32 host cloud.                                    */
int octl_forest_extend_pose_f32(octl_forest* f, int32_t slot, const float* xyz, int64_t n);
/* The same from a device pointer: octl_forest_extend_pose_device.                                              */
int octl_forest_extend_pose_device_f32(octl_forest* f, int32_t slot, const float* xyz_dev, int64_t n);

/* Clouds inserted UNDER A TRANSFORM: row i of the cloud is stored as ((R_i0 x + R_i1 y) + R_i2 z) + t_i of its own
 * 3x4 - every product and sum rounded to f64, no fused multiply-add (registration.py: transform_rows_np; an f32 row is
 * widened first) - so the forest holds exactly what the entry without a transform leaves for the cloud that was
 * transformed on the host: store, voxel box, domain flag, and with them every table and error of a later call.  A row
 * moved outside the domain fails at the build (OCTL_E_DOMAIN), as its host-transformed twin does, not here.
 *   flags         OCTL_XF_F32: xyz is (n,3) float; OCTL_XF_DEVICE: xyz is a device pointer (consumed in stream order,
 *                 ordered behind an octl_dev_upload_async into it, never read in place; 8-byte aligned for f64, 4-byte
 *                 for f32 is enough)
 *   transforms    HOST, n_transforms x 12 doubles: the rows (R_i0 R_i1 R_i2 t_i) of each 3x4.  Rigidity is not checked.
 *   segment       HOST uint16[n], or NULL with n_transforms == 1: the transform of every row ("piecewise rigid": the
 *                 firing columns of a sweep, each with its pose).  The caller has validated segment[i] < n_transforms;
 *                 the kernel clamps a larger index to n_transforms - 1 so that no read leaves the table.
 * All host buffers are the caller's again when the call returns.  OCTL_E_INVALID: n_transforms < 1 or
 * > OCTL_XF_MAX_SEGMENTS, n_transforms > 1 without a segment, a null buffer with n > 0, a transform that is not finite.
 * n == 0 launches nothing and still creates the pose.  One kernel whatever n; a host cloud costs one host wait, a
 * device cloud none.                                                                                              */
#define OCTL_XF_MAX_SEGMENTS 1024
enum { OCTL_XF_F32 = 1, OCTL_XF_DEVICE = 2 };
/* Grid.insert_points (grid/grid.py:58-109), OctreeManager.insert_points (octree_manager.py:161-171) and
 * Octree.insert_points (octree/octree.py:235-239, OctreeNode.insert_points octree/octree.py:67-100) of the transformed
 * cloud: octl_forest_add_pose.                                                                                   */
int octl_forest_add_pose_xf(octl_forest* f, const void* xyz, int64_t n, uint32_t flags, const double* transforms,
                            int32_t n_transforms, const uint16_t* segment, int32_t* slot);
/* OctreeManager.insert_points on an existing pose and Octree.insert_points (grid/grid.py:58-109 reaches them per
 * voxel; octree/octree.py:67-100) of the transformed cloud: octl_forest_extend_pose.                             */
int octl_forest_extend_pose_xf(octl_forest* f, int32_t slot, const void* xyz, int64_t n, uint32_t flags,
                               const double* transforms, int32_t n_transforms, const uint16_t* segment);

typedef struct octl_build_info {
  int64_t n_points;     /* alive points that were placed                                   */
  int64_t n_voxels;     /* top-level voxels (roots)                                        */
  int64_t n_nodes;      /* all scheme nodes: roots + 8 per internal node                   */
  int64_t n_internal;   /* internal scheme nodes                                           */
  int64_t n_blocks;     /* non-empty (leaf, pose) blocks                                   */
  int32_t max_depth;    /* deepest leaf                                                    */
  int32_t n_levels;     /* subdivision levels executed                                     */
} octl_build_info;

/* Build the scheme for the count criterion len(points) > K over the union of the poses
 * whose scheme_mask[slot] != 0 (NULL = all poses), then place every alive point of every
 * pose in its scheme leaf.  keep_scheme != 0 places the points in the EXISTING scheme
 * (a pose inserted after a subdivide inherits it, octree_manager.py:161-171) and ignores
 * K / scheme_mask: when whole poses were appended since the last build only their points are
 * placed and appended behind the leaf-ordered arrays (cost independent of what is stored);
 * after octl_forest_extend_pose / octl_forest_set_scheme every point is placed again.  K < 0 means "never split" (the state right after insert_points).
 * max_depth guards the recursion the reference does not bound (<= 0: default 63).
 * On OCTL_E_DOMAIN / OCTL_E_DEPTH / OCTL_E_NOMEM / OCTL_E_HIP the forest keeps its points and
 * voxels but is left without a scheme (the next build starts from the top-level voxels).
 * Streams: everything the build enqueues is ordered by the context's stream, as every call of the library is.  A
 * build of the route a scan loop takes - one pose read in place (octl_forest_add_pose_adopt) into a fresh scheme,
 * under the key geometry of the context's previous build - may put its first kernels (the partition of the cloud) on
 * a second stream of the context, where they run NEXT TO octl_forest_ransac_all / octl_forest_apply_mask(_async) of
 * the context's previous scan that are still in flight: those kernels read only the adopted cloud and write only
 * scratch of the build.  Before the call returns the context's stream has been made to wait for them, on error
 * returns too, so that on return nothing is in flight that the context's stream does not cover: octl_ctx_sync, a
 * later octl_dev_upload_async into the cloud's buffer and octl_dev_free behave as they always did.  The build stays
 * on the one stream whenever anything else was enqueued on the context since the forest's previous build, while the
 * context is profiling, below OCTL_BUILD_AHEAD_MIN_POINTS points, and with OCTL_NO_BUILD_AHEAD=1; results, launches
 * and host waits are the same either way.                                                              */
int octl_forest_build(octl_forest* f, int64_t K, const uint8_t* scheme_mask, int32_t n_mask,
                      int32_t keep_scheme, int32_t max_depth, octl_build_info* info);

/* octl_forest_build with a second split rule, evaluated on the device: a node splits when its scheme-pose count
 * exceeds K (K < 0: no count rule) OR it holds at least min_points scheme points and the smallest eigenvalue of
 * their covariance sum (p - mean)(p - mean)^T / (n - ddof) exceeds max_variance ("split while the points are not
 * flat"; octreelib_amd.NotPlanar is the same predicate as a host callable).  Scheme over the union of the poses of
 * scheme_mask, then every pose is placed; the result is an ordinary scheme (keep_scheme builds, late poses, RANSAC,
 * leaf_stats, masks work on it unchanged).  max_variance must be finite and > 0 - a cube of edge e cannot hold
 * points with a statistic above e^2 / 3, which bounds the depth whatever the points - min_points >= 4, ddof 0 or 1:
 * OCTL_E_INVALID otherwise.  Errors and what they leave behind as octl_forest_build.                            */
int octl_forest_build_planar(octl_forest* f, int64_t K, double max_variance, int32_t min_points, int32_t ddof,
                             const uint8_t* scheme_mask, int32_t n_mask, int32_t max_depth, octl_build_info* info);
/* Why the nodes of the last octl_forest_build_planar split: per scheme node (indexed like octl_forest_get_nodes)
 * the scheme-point count and the statistic the decision compared with max_variance - NaN where none was evaluated
 * (fewer than min_points scheme points).  Node i is internal iff n_scheme[i] > K or (n_scheme[i] >= min_points and
 * lambda_min[i] > max_variance).  Kept while the node table is the one that build left (placements into the scheme
 * that add no voxel keep it); for any other scheme n_scheme is 0 and lambda_min NaN everywhere.  Either output may
 * be NULL; size query with cap = 0.                                                                            */
int octl_forest_get_split_stats(octl_forest* f, int64_t cap, uint32_t* n_scheme, double* lambda_min,
                                int64_t* n_nodes);

/* Install a host-defined subdivision scheme (for criteria that are arbitrary host callables,
 * octree.py:26: the host decides which nodes split, the device does the placement): nodes
 * [0,V) are the roots in voxel order, the 8 children of node i are first_child[i]..+7 (-1 =
 * leaf), epoch[i] = build at which node i became internal.  Follow with
 * octl_forest_build(keep_scheme = 1) to place every point in this scheme.                     */
int octl_forest_set_scheme(octl_forest* f, const int32_t* first_child, const int32_t* epoch,
                           int64_t n_nodes, int32_t new_epoch);

/* ---- results of the last build (host copies; size-query = pass NULL outputs) ---------- */

/* Scheme nodes.  For node i: voxel (root) index, depth, parent (-1 for roots), first child
 * (-1 for leaves; children are first_child..first_child+7 in child_id order, child_id =
 * 4*ix+2*iy+iz as octree.py:94-97), corner_min[3] and edge_length computed with the
 * reference's arithmetic (octree.py:181-191), epoch = build call at which the node became
 * internal (0 for leaves).  Any output pointer may be NULL.                                */
int octl_forest_get_nodes(octl_forest* f, int64_t cap, int32_t* voxel, int32_t* depth,
                          int32_t* parent, int32_t* first_child, double* corner,
                          double* edge, int32_t* epoch, int64_t* n_nodes);
/* Integer coordinates of the top-level voxels, (V,3) int64, lexicographically sorted — the
 * order of np.unique(axis=0) at grid.py:79-81.                                            */
int octl_forest_get_voxels(octl_forest* f, int64_t cap, int64_t* coords, int64_t* n_voxels);
/* Non-empty (leaf, pose) blocks in storage order (voxel, leaf path, pose): scheme node id of
 * the leaf, pose slot, start and size in the leaf-ordered arrays.                          */
int octl_forest_get_blocks(octl_forest* f, int64_t cap, int32_t* node, int32_t* slot,
                           int64_t* start, int32_t* size, int64_t* n_blocks);
/* Ranks (indices into the voxel table, ascending) of the top-level voxels in which a pose slot
 * currently has points - Grid.__pose_voxel_coordinates (grid.py:53,108) without fetching the
 * node and block tables.                                                                     */
int octl_forest_get_slot_voxels(octl_forest* f, int32_t slot, int64_t cap, int32_t* voxel_ranks,
                                int64_t* n);
/* Counters of one pose without fetching the tables (octree.py:144-175, octree_manager.py:132-159,
 * grid.py:343-362): points and non-empty leaves of the slot, reduced on the device ...            */
int octl_forest_slot_counts(octl_forest* f, int32_t slot, int64_t* n_points, int64_t* n_leaves);
/* ... and the internal scheme nodes of every top-level voxel (V int32): n_nodes of a pose is the sum of
 * 1 + 8 * internal over the voxels the pose was inserted into.                                     */
int octl_forest_internal_per_voxel(octl_forest* f, int64_t cap, int32_t* counts, int64_t* n_voxels);
/* Leaf-ordered point permutation: perm[i] = index of the point at storage position i in
 * the concatenation of all pose clouds in slot order (pose-local index = perm - offset of
 * its slot).  Within a block the order is ascending (stable).                              */
int octl_forest_get_perm(octl_forest* f, int64_t cap, int64_t* perm, int64_t* n);
/* Leaf-ordered coordinates (n,3) f64 for storage positions [start, start+count).           */
int octl_forest_get_points(octl_forest* f, int64_t start, int64_t count, double* xyz);
/* The rows of the blocks block_ids[0..m) (host array), concatenated in THAT order: one device gather and one
 * download instead of a host loop over the blocks.  *n_points = rows of the selection; rows are written only when
 * xyz != NULL and cap >= *n_points (call with xyz = NULL for the size).  Replaces the concatenation loops of
 * Grid.get_points / OctreeManager.get_points / Octree.get_points (grid.py:234-242, octree_manager.py:121-130,
 * octree.py:55-65,252-254), whose order - managers in creation order, leaves in cached order - the caller encodes
 * in block_ids.                                                                                                */
int octl_forest_gather_blocks(octl_forest* f, const int32_t* block_ids, int64_t m, int64_t cap, double* xyz,
                              int64_t* n_points);
/* Per-(leaf, pose) point statistics over the blocks block_ids[0..nb) (indices into the block table), outputs
 * indexed like block_ids, any may be NULL: count (nb) i64, mean (nb,3), cov (nb,6) upper triangle xx xy xz yy yz zz
 * of the population covariance, eigval (nb,3) ascending, eigvec (nb,3,3) columns = eigenvectors. Read-only: the
 * forest, its caches, a pending RANSAC mask are untouched. OCTL_E_STATE before the first build, OCTL_E_INVALID for an
 * id outside [0, n_blocks).                                                                                       */
int octl_forest_leaf_stats(octl_forest* f, const int32_t* block_ids, int64_t nb, int64_t* count, double* mean,
                           double* cov, double* eigval, double* eigvec);
/* One plane per LEAF over a set of poses (a map plane pools the poses that observed the leaf): for every leaf that
 * holds at least one point of the poses with slot_sel[slot] != 0 (NULL: all poses; otherwise n_sel = number of poses),
 * in ascending node id (the row index of octl_forest_get_nodes), the node, the count, mean, population covariance
 * (6 upper-triangle values) and eigen-decomposition - conventions, sign rule and solver of octl_forest_leaf_stats - of
 * ALL its points of those poses together.  *n_leaves = number of such leaves; rows are written only when cap >=
 * *n_leaves (size query: cap = 0); any output may be NULL.  Arithmetic: anchor a = the leaf's centre (corner + edge/2),
 * every (leaf, pose) block's sums of d = p - a and d d^T by the chunked wave reduction of octl_forest_leaf_stats, the
 * blocks added in ascending slot order.  With B pooled blocks, the largest of n_max points, g = (ceil(n_max / 64) +
 * ceil(n_max / 4096) + B + 16) * 2^-53 and R = max |p - a|_inf over the pooled points: mean within 2 g R + 2^-53 |mean|,
 * every covariance entry within 4 g R^2 of the exact value; eigenvalues within 64 * 2^-53 * |C|_F of those of the
 * returned covariance.  A leaf's bits depend on its own points and on the selection only.  The table also stays on
 * the device for octl_forest_point_to_plane, until a call changes the forest's contents or scheme (build*, add_pose*,
 * extend_pose*, apply_mask*, apply_host_mask, filter_count, carve*, remove_sparse, set_contents, set_scheme, clear).  Read-only
 * otherwise.
 * OCTL_E_STATE before the first build.  No reference counterpart (the reference has no per-leaf statistics).        */
int octl_forest_pooled_leaf_stats(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int64_t cap, int32_t* node,
                                  int64_t* count, double* mean, double* cov6, double* eigval, double* eigvec,
                                  int64_t* n_leaves);
/* Which leaf of the scheme does each of n query points (n,3) f64 fall into?  node[i] = id (row of
 * octl_forest_get_nodes) of the leaf whose cube contains point i, found exactly as the point of a late pose is placed
 * (voxel by floor division, root by binary search over the sorted voxel keys, descent by the reference's child-index
 * comparisons, octree/octree.py:67-100); -1 for a point whose top-level voxel the scheme does not hold, that lies
 * outside the single cube of a mode-1 forest or outside the cube of a split node, outside the voxel domain, or is not
 * finite.  Such a point raises nothing and leaves octl_last_error alone.  Read-only: tables, store, counters, a
 * pending mask are untouched; an unsubdivided forest answers with root nodes.  One kernel (plus the voxel-key sync the
 * first time after a build); the host form adds one upload, one download and one wait.  OCTL_E_STATE before the
 * first build.  No reference counterpart: the reference can only insert the points, which changes the tree.        */
int octl_forest_locate(octl_forest* f, const double* xyz, int64_t n, int32_t* node);
/* The same with pointers from octl_dev_alloc: nothing is downloaded and the host does not wait (the answer is
 * complete in stream order: octl_dev_download / octl_ctx_sync).  No reference counterpart.                        */
int octl_forest_locate_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t* node_dev);
/* octl_forest_locate fused with the plane of the leaf in the table of the last octl_forest_pooled_leaf_stats
 * (OCTL_E_STATE, with a message that names the cause, if there is none or the forest has changed since): row[i] =
 * row of that table, or -1 when node[i] < 0, the leaf holds no pooled point, fewer than min_points of them, or (when
 * max_variance >= 0) a smallest eigenvalue above max_variance; distance[i] = the signed distance
 * fma(nx, dx, fma(ny, dy, nz * dz)), d = p - mean, n = the smallest eigenvalue's vector, NaN where row[i] < 0.  Given
 * the table's own plane bits the result is within 4 * 2^-53 * (|nx dx| + |ny dy| + |nz dz|) of the exact value.
 * One kernel; the host form adds one upload, three downloads and one wait.  No reference counterpart.              */
int octl_forest_point_to_plane(octl_forest* f, const double* xyz, int64_t n, int32_t min_points, double max_variance,
                               int32_t* node, int32_t* row, double* distance);
/* The same with pointers from octl_dev_alloc; no host wait.  No reference counterpart.                             */
int octl_forest_point_to_plane_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t min_points,
                                      double max_variance, int32_t* node_dev, int32_t* row_dev,
                                      double* distance_dev);
/* The stored points nearest to every query point, within max_distance: exact k-nearest neighbours across leaf walls.
 * For query q and stored point p: dx = q_x - p_x (dy, dz likewise), d2 = (dx dx + dy dy) + dz dz in f64 with every
 * product and sum rounded (no fma).  Candidates are the points of the selected poses (slot_sel: n_sel = number of
 * poses flags, NULL = every pose) that are alive and in the leaf-ordered arrays - what a mask or filter removed is
 * never returned - with d2 <= max_distance * max_distance (inclusive).  Row i of the (n, k) outputs holds the k best
 * in ascending (d2, slot, index): slot_out = the pose slot, index_out = the point's row in that pose's cloud as it
 * was inserted (the value of octl_forest_get_perm minus the pose's offset; masks and filters do not renumber it),
 * d2_out = d2; places beyond count_out[i] <= k hold -1, -1, +inf.  A query with a coordinate that is not finite has
 * count 0.  The order is total, so the answer is a function of the input: octreelib_amd/query.py: nearest_np is the
 * same by brute force, bit for bit.
 * OCTL_E_INVALID: k outside 1 .. OCTL_NN_MAX_K; max_distance not finite or <= 0; a grid with max_distance above twice
 * the voxel edge (a query would touch more than 5 voxels per axis: the cap bounds a call's cost).  OCTL_E_STATE:
 * before the first build; a forest whose rows map_leaf_points moved outside their leaves (octl_forest_set_contents),
 * where no cube bounds what it holds.  The index of the blocks by node is made by the call that finds it missing,
 * stale or made for another selection (a few launches and one wait); with it in place a call is one kernel, plus
 * one upload, the downloads and one wait.  No reference counterpart.                                              */
#define OCTL_NN_MAX_K 8
int octl_forest_nearest(octl_forest* f, const double* xyz, int64_t n, int32_t k, double max_distance,
                        const uint8_t* slot_sel, int32_t n_sel, int32_t* slot_out, int64_t* index_out, double* d2_out,
                        int32_t* count_out);
/* The same with pointers from octl_dev_alloc (slot_sel stays a host array): one kernel, nothing is downloaded and
 * the host does not wait.  No reference counterpart.                                                             */
int octl_forest_nearest_device(octl_forest* f, const double* xyz_dev, int64_t n, int32_t k, double max_distance,
                               const uint8_t* slot_sel, int32_t n_sel, int32_t* slot_dev, int64_t* index_dev,
                               double* d2_dev, int32_t* count_dev);
/* What does a ray hit first?  For each of n rays o + t d, t_min <= t <= t_max (origins, directions (n,3) f64, t_min,
 * t_max (n) f64; directions are taken as given - t is the ray parameter, a distance only for unit vectors): the first
 * occupied leaf (surface = OCTL_RAY_CUBE) or the first accepted pooled plane (OCTL_RAY_PLANE) of the selected poses
 * (slot_sel: n_sel = number of poses flags, NULL = every pose).  octreelib_amd/query.py: raycast_np is the same by
 * brute force over the leaves, bit for bit; all arithmetic in f64, every product, sum and quotient rounded (no fma):
 *   dead ray   any of o, d, t_min, t_max not finite; t_max < t_min; a component with |d| > 1; every component of d zero
 *              or with a reciprocal that is not finite.  Answer node -1, t +inf, row -1; never an error;
 *   interval   of the leaf (corner c, edge e), lo = c, hi = fl(c + e): an axis whose d is zero or whose inv = fl(1 / d)
 *              is not finite passes iff lo <= o <= hi and bounds nothing; otherwise a = fl(fl(lo - o) inv), b =
 *              fl(fl(hi - o) inv), near = min(a, b), far = max(a, b).  t_in = max(near_x, near_y, near_z, t_min), t_out
 *              = min(far_x, far_y, far_z, t_max); the leaf is crossed iff every such axis passes and t_in <= t_out;
 *   cube       candidates: crossed scheme leaves (never inner nodes) that hold at least min_points points of the
 *              selection that are alive and in the leaf-ordered arrays; t = t_in;
 *   plane      candidates: crossed leaves whose row of the pooled table passes octl_forest_point_to_plane's gates
 *              (count >= min_points and, with max_variance >= 0, not lambda0 > max_variance), with num = (nx fl(mx -
 *              ox) + ny fl(my - oy)) + nz fl(mz - oz), den = (nx dx + ny dy) + nz dz, t = fl(num / den), den != 0 and
 *              t_in <= t <= t_out (n the eigenvector of lambda0, m the mean, the table's own bits);
 *   answer     the candidate smallest in (t, node): node[i] its id, t[i] its t, row[i] its row of the pooled table
 *              (plane) or -1 (cube).  The order is total, so the answer is a function of the input.
 * A grid caps a ray that is not dead at t_max - t_min <= 256 voxel edges and |t_min|, |t_max| <= 2^40 voxel edges
 * (the cap bounds a call's cost; a 1 m grid answers 256 m rays): OCTL_E_INVALID above it.  A single cube has no cap.
 * OCTL_E_INVALID also: a surface that is neither, min_points < 0, max_variance NaN, a selection of the wrong length.
 * OCTL_E_STATE: before the first build; a forest whose rows map_leaf_points moved outside their leaves.  The tables
 * a call reads - the index of the blocks by node of octl_forest_nearest (cube), the pooled planes (plane) - are made
 * by the call that finds them missing, stale or made for another selection; with them in place a call is one kernel,
 * plus four uploads, three downloads and one wait.  Read-only otherwise.  No reference counterpart.              */
#define OCTL_RAY_CUBE 0
#define OCTL_RAY_PLANE 1
int octl_forest_raycast(octl_forest* f, const double* origins, const double* directions, const double* t_min,
                        const double* t_max, int64_t n, const uint8_t* slot_sel, int32_t n_sel, int32_t surface,
                        int32_t min_points, double max_variance, int32_t* node, double* t, int32_t* row);
/* The same with pointers from octl_dev_alloc (slot_sel stays a host array): one kernel, nothing is downloaded and
 * the host does not wait.  The cap cannot be checked without reading the rays: one above it is answered as a dead
 * ray is.  No reference counterpart.                                                                              */
int octl_forest_raycast_device(octl_forest* f, const double* origins_dev, const double* directions_dev,
                               const double* t_min_dev, const double* t_max_dev, int64_t n, const uint8_t* slot_sel,
                               int32_t n_sel, int32_t surface, int32_t min_points, double max_variance,
                               int32_t* node_dev, double* t_dev, int32_t* row_dev);
/* Ray evidence per leaf: how many of n rays END in each leaf of the scheme and how many only pass THROUGH it - the
 * free-space evidence a map is kept clean with (octl_forest_carve).  Per ray o, d (taken as given), t_min, t_free, t_end
 * ((n,3), (n,3), (n) f64): the free interval F = [t_min, t_free] (empty when t_free < t_min) and the end interval E =
 * [e0, t_end] with e0 = max(t_min, t_free) (empty when t_end < e0); for a measured range r and a margin m a caller
 * passes t_free = fl(r - m), t_end = fl(r + m).  octreelib_amd/query.py: ray_evidence_np is the same by brute force
 * over the leaves, equal count for count; all arithmetic in f64, every product, sum and quotient rounded (no fma):
 *   dead ray   any of o, d, t_min, t_free, t_end not finite; a component with |d| > 1; every component of d zero or with
 *              a reciprocal that is not finite.  It adds nothing; never an error;
 *   per leaf   near, far per axis and the pass test of an axis that bounds nothing as octl_forest_raycast's interval;
 *              near = max over the bounding axes (-inf: none), far = min (+inf: none);
 *              in_E iff every axis passes and max(near, e0) <= min(far, t_end);
 *              in_F iff every axis passes and max(near, t_min) <= min(far, t_free)   (both ends inclusive);
 *   answer     hits[v] = rays with in_E, through[v] = rays with in_F and not in_E, for every node v (row of
 *              octl_forest_get_nodes), u32; inner nodes hold 0.
 * A function of the scheme and the rays alone: no occupancy, no pose selection, so it also answers for a forest whose
 * rows map_leaf_points moved outside their leaves.  *n_nodes = the scheme's node count; the counters are written only
 * when cap_nodes >= *n_nodes (size query: cap_nodes = 0).  n = 0: zeros, no kernel.  A grid caps a ray whose t are
 * finite at max(t_free, t_end) - t_min <= 256 voxel edges and |t_min|, |max(t_free, t_end)| <= 2^40 voxel edges, as
 * octl_forest_raycast does: OCTL_E_INVALID above it.  OCTL_E_INVALID also: n < 0 or >= 2^31, a NULL array with n > 0.
 * OCTL_E_STATE before the first build.  Five uploads, one fill of both counters, one kernel (each ray walks every leaf
 * it crosses once and does one u32 atomic add there), two downloads, one wait.  Read-only.  No reference counterpart. */
int octl_forest_ray_evidence(octl_forest* f, const double* origins, const double* directions, const double* t_min,
                             const double* t_free, const double* t_end, int64_t n, int64_t cap_nodes, uint32_t* through,
                             uint32_t* hits, int64_t* n_nodes);
/* The same with pointers from octl_dev_alloc: one kernel that ADDS into the caller's through_dev / hits_dev of n_nodes
 * u32 each (OCTL_E_INVALID unless n_nodes is the scheme's node count) - the caller zeroes them, and may accumulate
 * several scans; a counter wraps at 2^32, which is the caller's concern.  Nothing is downloaded and the host does not
 * wait.  The cap cannot be checked without reading the rays: a ray above it adds nothing.  No reference counterpart. */
int octl_forest_ray_evidence_device(octl_forest* f, const double* origins_dev, const double* directions_dev,
                                    const double* t_min_dev, const double* t_free_dev, const double* t_end_dev,
                                    int64_t n, uint32_t* through_dev, uint32_t* hits_dev, int64_t n_nodes);
/* Remove what rays saw through: every (leaf, pose) block of a pose with slot_sel[slot] != 0 (NULL: every pose; otherwise
 * n_sel = number of poses) whose leaf has through[node] >= min_through and hits[node] <= max_hits loses all its points
 * (octreelib_amd/query.py: carve_keep_np is the rule; through, hits: n_nodes u32 each, the counters of
 * octl_forest_ray_evidence - evidence belongs to the scheme it was taken on).  The blocks are cleared in the mask and
 * the mask is applied as octl_forest_filter_count applies its own: a pending RANSAC mask goes into the same ONE
 * compaction.  The scheme stays; *n_alive (nullable) = points left in the leaf-ordered arrays.  OCTL_E_INVALID: n_nodes
 * is not the scheme's node count, a NULL counter array, a selection of the wrong length, min_through < 1, max_hits < 0.
 * OCTL_E_STATE before the first build.  Two uploads, one kernel, the compaction.  No reference counterpart.          */
int octl_forest_carve(octl_forest* f, const uint32_t* through, const uint32_t* hits, int64_t n_nodes,
                      const uint8_t* slot_sel, int32_t n_sel, int64_t min_through, int64_t max_hits, int64_t* n_alive);
/* The same with the counters in device memory (pointers from octl_dev_alloc, as octl_forest_ray_evidence_device left
 * them: nothing is downloaded).  No reference counterpart.                                                          */
int octl_forest_carve_device(octl_forest* f, const uint32_t* through_dev, const uint32_t* hits_dev, int64_t n_nodes,
                             const uint8_t* slot_sel, int32_t n_sel, int64_t min_through, int64_t max_hits,
                             int64_t* n_alive);
/* How many stored points lie within `radius` of every query point?  For query q and stored point p: d2 as
 * octl_forest_nearest forms it (dx = q_x - p_x, d2 = (dx dx + dy dy) + dz dz in f64, every product and sum rounded, no
 * fma); p counts iff d2 <= radius * radius (formed once, inclusive) - exactly the candidates of octl_forest_nearest, of
 * the same points: those of the selected poses (slot_sel: n_sel = number of poses flags, NULL = every pose) that are
 * alive and in the leaf-ordered arrays; what a mask, a filter, carve or remove_poses took out never counts.  count[i] =
 * min(number of counting points, max_count), int32; max_count = 0: uncapped.  A query with a coordinate that is not
 * finite counts 0.  octreelib_amd/query.py: radius_count_np is the same by brute force, count for count.  The search
 * is the walk of octl_forest_nearest with a sink that counts; a capped query stops at the cap.
 * OCTL_E_INVALID: max_count < 0; radius not finite or <= 0; a grid with radius above twice the voxel edge; n < 0 or
 * >= 2^31; a NULL array with n > 0; a selection of the wrong length.  OCTL_E_STATE: before the first build; a forest
 * whose rows map_leaf_points moved outside their leaves.  All before anything runs.  n = 0 returns without a kernel.
 * The index of the blocks by node (octl_forest_nearest's own, under its stamp) is made by the call that finds it
 * missing, stale or made for another selection; with it in place a call is one kernel, plus one upload, one download
 * and one wait.  Read-only otherwise.  No reference counterpart.                                                   */
int octl_forest_radius_count(octl_forest* f, const double* xyz, int64_t n, double radius, int32_t max_count,
                             const uint8_t* slot_sel, int32_t n_sel, int32_t* count);
/* The same with pointers from octl_dev_alloc (slot_sel stays a host array): one kernel, nothing is downloaded and
 * the host does not wait.  No reference counterpart.                                                             */
int octl_forest_radius_count_device(octl_forest* f, const double* xyz_dev, int64_t n, double radius, int32_t max_count,
                                    const uint8_t* slot_sel, int32_t n_sel, int32_t* count_dev);
/* Radius outlier removal: every point x of the leaf-ordered arrays that belongs to a tested pose (slot_sel[slot] != 0;
 * NULL: every pose; otherwise n_sel = number of poses) and has fewer than min_neighbours OTHER points of the counted
 * poses (among_sel / n_among likewise) within `radius` is removed.  c(x) = the stored points y of the counted poses
 * with d2(x, y) <= radius * radius, d2 as octl_forest_radius_count forms it with q = the stored bits of x, and y != x
 * decided by identity (pose, row), not by distance: a duplicate at the same coordinates is a neighbour, and a tested
 * pose that is not counted loses nothing to itself.  keep(x) iff c(x) >= min_neighbours (the count saturates there).
 * Every decision is made on the map as it is before the call - one simultaneous round, not idempotent: a second
 * call may remove more.  octreelib_amd/query.py: sparse_keep_np is the rule.  Points that a pending RANSAC mask is
 * about to drop are still in the ordered arrays: they count as neighbours and are judged (octl_forest_filter_count's
 * rule).  The kernel clears bytes in the mask and the mask is applied as octl_forest_carve applies its own: a pending
 * RANSAC mask goes into the same ONE compaction.  The scheme stays (voxels and leaves that lose every point stay,
 * empty: octl_forest_prune drops them); the index of octl_forest_nearest of a surviving row is unchanged; the block
 * index, the pooled planes, the segments and the adjustment tables go stale as after octl_forest_carve.  *n_alive
 * (nullable) = points left in the leaf-ordered arrays.
 * OCTL_E_INVALID: min_neighbours < 1; radius not finite or <= 0; a grid with radius above twice the voxel edge; a
 * selection of the wrong length.  OCTL_E_STATE: before the first build; a forest whose rows map_leaf_points moved
 * outside their leaves.  All before anything runs: a refused call leaves points and mask as they were, and every
 * buffer is reserved before the mask is written.  One wavefront per (leaf, pose) block; with the index of among_sel
 * in place a call is one kernel (which also writes the ones of a mask that was not pending) and the compaction, plus
 * one upload and one wait for a tested selection.  No reference counterpart.                                        */
int octl_forest_remove_sparse(octl_forest* f, double radius, int32_t min_neighbours, const uint8_t* slot_sel,
                              int32_t n_sel, const uint8_t* among_sel, int32_t n_among, int64_t* n_alive);
/* How many stored points lie in the lattice cell of every query point?  The lattice is absolute (origin 0, nothing to
 * do with the subdivision): the cell of p is floor(p / cell) per axis, the floor of the TRUE quotient as
 * np.floor_divide forms it, and two points share a cell iff the three indices are equal.  The counted points are those
 * of octl_forest_radius_count: of the selected poses (slot_sel: n_sel = number of poses flags, NULL = every pose),
 * alive and in the leaf-ordered arrays.  count[i] = min(number of stored points of the cell, max_count), int32;
 * max_count = 0: uncapped.  A query with a coordinate that is not finite counts 0.  octreelib_amd/thinning.py:
 * cell_count_np is the same by hashing, count for count.  The search is the stackless walk of octl_forest_nearest with
 * a box prune and a sink that counts; membership is decided on the signs of two fused remainders, without a division;
 * a capped query stops at the cap.
 * OCTL_E_INVALID: max_count < 0; cell not finite or <= 0; a grid with cell above the voxel edge L or below L 2^-20, a
 * single cube with max(|corner|, |corner + edge|) / cell >= 2^50 (every cell index of the map's domain stays an exact
 * double); n < 0 or >= 2^31; a NULL array with n > 0; a selection of the wrong length.  OCTL_E_STATE: before the first
 * build; a forest whose rows map_leaf_points moved outside their leaves.  All before anything runs.  n = 0 returns
 * without a kernel.  The index of the blocks by node (octl_forest_nearest's own, under its stamp) is made by the call
 * that finds it missing, stale or made for another selection; with it in place a call is one kernel, plus one upload,
 * one download and one wait.  Read-only otherwise.  No reference counterpart.                                       */
int octl_forest_cell_count(octl_forest* f, const double* xyz, int64_t n, double cell, int32_t max_count,
                           const uint8_t* slot_sel, int32_t n_sel, int32_t* count);
/* The same with pointers from octl_dev_alloc (slot_sel stays a host array): one kernel, nothing is downloaded and
 * the host does not wait.  No reference counterpart.                                                             */
int octl_forest_cell_count_device(octl_forest* f, const double* xyz_dev, int64_t n, double cell, int32_t max_count,
                                  const uint8_t* slot_sel, int32_t n_sel, int32_t* count_dev);
/* Voxel-grid thinning: of the points of the leaf-ordered arrays that share a lattice cell (octl_forest_cell_count's
 * cells) only the first max_per_cell stay.  The order is that of the point store: poses in slot order, rows in
 * insertion order - the (slot, index) order of octl_forest_nearest.  For a point x of a tested pose (slot_sel[slot]
 * != 0; NULL: every pose; otherwise n_sel = number of poses), rank(x) = the stored points y of the counted poses
 * (among_sel / n_among likewise) in the cell of x that come BEFORE x in that order: x never counts itself, an earlier
 * duplicate at the same coordinates does, and a tested pose that is not counted is judged against the counted ones
 * only.  keep(x) iff rank(x) < max_per_cell (the count saturates there).  Every decision is made on the map as it is
 * before the call - one simultaneous round; with every pose tested and counted it keeps exactly the first
 * max_per_cell points of every cell and a second call removes nothing.  octreelib_amd/thinning.py: thin_keep_np is
 * the rule.  Points that a pending RANSAC mask is about to drop are still in the ordered arrays: they occupy cells and
 * are judged (the kernel never reads the mask).  The kernel clears bytes in the mask and the mask is applied as
 * octl_forest_remove_sparse applies its own: a pending RANSAC mask goes into the same ONE compaction.  The scheme
 * stays; the index of octl_forest_nearest of a surviving row is unchanged; the block index, the pooled planes, the
 * segments and the adjustment tables go stale.  *n_alive (nullable) = points left in the leaf-ordered arrays.
 * OCTL_E_INVALID: max_per_cell < 1; cell as octl_forest_cell_count refuses it; a selection of the wrong length.
 * OCTL_E_STATE: before the first build; a forest whose rows map_leaf_points moved outside their leaves.  All before
 * anything runs: a refused call leaves points and mask as they were, and every buffer is reserved before the mask is
 * written.  One wavefront per (leaf, pose) block; with the index of among_sel in place a call is one kernel (which
 * also writes the ones of a mask that was not pending) and the compaction, plus one upload and one wait for a tested
 * selection.  No reference counterpart.                                                                            */
int octl_forest_thin(octl_forest* f, double cell, int32_t max_per_cell, const uint8_t* slot_sel, int32_t n_sel,
                     const uint8_t* among_sel, int32_t n_among, int64_t* n_alive);
/* What the surface looks like round every query point: count, mean, population covariance (6 upper-triangle values xx
 * xy xz yy yz zz) and its eigen-decomposition - conventions, sign rule and solver of octl_forest_leaf_stats - of the
 * stored points within `radius`.  The neighbours are exactly the points octl_forest_radius_count counts, uncapped: the
 * same walk, the same d2 bits, the same inclusive d2 <= radius * radius, the same selection (slot_sel: n_sel = number
 * of poses flags, NULL = every pose), so count[i] is its count.  Arithmetic: the sums of d = fl(p - q) and of d d^T
 * (fma) in f64, one neighbour after the other in the order of the walk, then mean = q + S_d / n and cov = S_dd / n -
 * (S_d / n)(S_d / n)^T; a single neighbour has covariance 0 exactly.  With n neighbours, R = max |p - q|_inf over them
 * and g = (n + 16) * 2^-53: mean within 2 g R + 2^-53 |mean|, every covariance entry within 4 g R^2 of the exact value
 * (the magnitude of the coordinates does not enter); eigenvalues within 64 * 2^-53 * |C|_F of those of the returned
 * covariance.  A row's bits depend on the forest's tables and on the query's bits only - not on the batch, not on
 * where the query lies in memory; another subdivision of the same points walks in another order and may differ within
 * the bound.  A query that is not finite, and one without a neighbour, has count 0 and NaN in every other field.
 * outputs: count (n) i64, mean (n,3), cov (n,6), eigval (n,3), eigvec (n,3,3) columns = eigenvectors; any may be NULL,
 * eigval and eigvec only together (both NULL: no decomposition).  octreelib_amd/neighbourhood.py:
 * neighbourhood_statistics_np is the definition.
 * OCTL_E_INVALID: radius not finite or <= 0; a grid with radius above twice the voxel edge; n < 0 or >= 2^31; xyz NULL
 * with n > 0; a selection of the wrong length.  OCTL_E_STATE: before the first build; a forest whose rows
 * map_leaf_points moved outside their leaves.  All before anything runs.  n = 0 returns without a kernel.  With the
 * index of the selection in place (octl_forest_nearest's own) a call is one kernel, plus one upload, the downloads and
 * one wait.  Read-only otherwise.  No reference counterpart.                                                        */
int octl_forest_neighbourhood_stats(octl_forest* f, const double* xyz, int64_t n, double radius,
                                    const uint8_t* slot_sel, int32_t n_sel, int64_t* count, double* mean, double* cov,
                                    double* eigval, double* eigvec);
/* The same with pointers from octl_dev_alloc (slot_sel stays a host array; count, mean and cov are required): one
 * kernel, nothing is downloaded and the host does not wait.  No reference counterpart.                           */
int octl_forest_neighbourhood_stats_device(octl_forest* f, const double* xyz_dev, int64_t n, double radius,
                                           const uint8_t* slot_sel, int32_t n_sel, int64_t* count_dev,
                                           double* mean_dev, double* cov_dev, double* eigval_dev, double* eigvec_dev);
/* The self-query: one row of octl_forest_neighbourhood_stats for every point of the leaf-ordered arrays that belongs
 * to a tested pose (slot_sel[slot] != 0; NULL: every pose; otherwise n_sel = number of poses), over the stored points
 * of the counted poses (among_sel / n_among likewise), with q = the stored bits of the point - the row
 * octl_forest_neighbourhood_stats gives for those bits under the selection among_sel, bit for bit.  The point counts
 * itself when its pose is counted (the opposite of octl_forest_remove_sparse).  Points that a pending RANSAC mask is
 * about to drop are still in the ordered arrays: they have rows and count.  slot[i], index[i] (int32) name the point
 * of row i: its pose's slot and its row in that pose's cloud as inserted (the index of octl_forest_nearest).  The
 * rows come in no particular order: the caller sorts them by (slot, index).  *n_rows = number of rows; they are
 * written only when cap >= *n_rows (size query: cap = 0), and a cap of at least min(ordered points, store rows of
 * the tested poses) saves the second wait.  Other outputs as above, any may be NULL.
 * OCTL_E_INVALID: cap < 0; n_rows NULL; radius as above; a selection of the wrong length.  OCTL_E_STATE as above.  One
 * wavefront per (leaf, pose) block; with the index of among_sel in place a call is one fill and one kernel, plus one
 * upload for a tested selection, the downloads and one wait (two when cap is below the bound).  Nothing of the forest
 * changes and no cached table is dropped.  No reference counterpart.                                              */
int octl_forest_point_stats(octl_forest* f, double radius, const uint8_t* slot_sel, int32_t n_sel,
                            const uint8_t* among_sel, int32_t n_among, int64_t cap, int64_t* n_rows, int32_t* slot,
                            int32_t* index, int64_t* count, double* mean, double* cov, double* eigval,
                            double* eigvec);
/* Euclidean cluster extraction: the connected components of "two stored points are within `radius` of each other" over
 * the points of the leaf-ordered arrays that belong to a selected pose (slot_sel[slot] != 0; NULL: every pose;
 * otherwise n_sel = number of poses).  Two points are joined iff d2 = (dx dx + dy dy) + dz dz <= radius^2 in f64 with
 * separate products and sums, inclusive - the candidates of octl_forest_radius_count under the same selection, found
 * by the same walk; a duplicate at the same coordinates is a neighbour.  The selected poses are the whole graph: points
 * of other poses have no row and bridge nothing.  Points that a pending RANSAC mask is about to drop are still in the
 * ordered arrays: they have rows and connect.  octreelib_amd/clustering.py: cluster_labels_np is the definition.
 * One row per vertex: slot[i], index[i] (int32) name the point (its pose's slot and its row in that pose's cloud as
 * inserted - the index of octl_forest_nearest), first[i] (int64) = slot << 32 | index of the smallest member of its
 * component in that order, size[i] (int32) the number of members.  The rows come in no particular order: the caller
 * sorts them by (slot, index) and numbers the distinct values of `first`.  *n_rows = number of rows; they are written
 * only when cap >= *n_rows (size query: cap = 0), and a cap of at least min(ordered points, store rows of the selected
 * poses) saves the second wait.  Any output array may be NULL.
 * OCTL_E_INVALID: cap < 0; n_rows NULL; radius not finite or <= 0; a grid with radius above twice the voxel edge; a
 * selection of the wrong length.  OCTL_E_STATE: before the first build; a forest whose rows map_leaf_points moved
 * outside their leaves; a union-find that ran out of its step budget (damaged tables).  One wavefront per (leaf, pose)
 * block; with the index of the selection in place a call is four kernels (init, link, flatten, rows), two small
 * uploads, the downloads and one wait (two when cap is below the bound), whatever the number of points, clusters or
 * path lengths.  The answer is a function of the stored points and the selection alone: not of the subdivision, the
 * layout or the schedule.  Nothing of the forest changes and no cached table is dropped.  No reference counterpart.  */
int octl_forest_cluster_points(octl_forest* f, double radius, const uint8_t* slot_sel, int32_t n_sel, int64_t cap,
                               int64_t* n_rows, int32_t* slot, int32_t* index, int64_t* first, int32_t* size);
/* Remove small clusters: every point of the selected poses whose component - octl_forest_cluster_points over the same
 * selection - has fewer than min_points members leaves the leaf-ordered arrays (and counts as removed in the store):
 * clumps of speckle that octl_forest_remove_sparse keeps because each of their points has neighbours.  Every decision
 * is made on the map as it is before the call - one simultaneous round, after which a second call removes nothing.
 * octreelib_amd/clustering.py: small_cluster_keep_np is the rule.  The kernels never read the mask: points a pending
 * RANSAC mask is about to drop still connect and are judged.  The kernel clears bytes in the mask and the mask is
 * applied as octl_forest_remove_sparse applies its own: a pending RANSAC mask goes into the same ONE compaction.  The
 * scheme stays; the index of octl_forest_nearest of a surviving row is unchanged; the block index, the pooled planes,
 * the segments and the adjustment tables go stale.  *n_alive (nullable) = points left in the leaf-ordered arrays.
 * OCTL_E_INVALID: min_points < 1; radius as above; a selection of the wrong length.  OCTL_E_STATE: before the first
 * build; a forest whose rows map_leaf_points moved outside their leaves - both before anything runs: a refused call
 * leaves points and mask as they were, and every buffer is reserved before the mask is written; a union-find that ran
 * out of its step budget (damaged tables) clears no byte of the mask and is reported after the compaction.  With the
 * index of the selection in place a call is four kernels (init, link, flatten, mask: it also writes the ones of a
 * mask that was not pending), two small uploads and the compaction with its one wait.  No reference counterpart.     */
int octl_forest_remove_small_clusters(octl_forest* f, double radius, int32_t min_points, const uint8_t* slot_sel,
                                      int32_t n_sel, int64_t* n_alive);
/* Plane segments: the rows of the pooled plane table (octl_forest_pooled_leaf_stats of the selection slot_sel; made by
 * this call when the forest holds none that is valid) merged across the faces of their leaves into connected coplanar
 * regions.  octreelib_amd/query.py: plane_segments_np is the definition; every decision is made on the table's bits in
 * f64 with every product and sum rounded (no fma), so neighbour, label, root and n_leaves EQUAL it.
 *   eligible   a row with count >= min_points, lambda0 finite and, with max_variance >= 0, lambda0 <= max_variance;
 *   neighbour  (rows, 6) node ids behind the faces -x +x -y +y -z +z: the leaf that holds the centre of the row's cube
 *              with one coordinate replaced by corner + edge (+) or by the double before corner (-), as
 *              octl_forest_locate answers; -1 for no leaf or the leaf itself;
 *   edge       rows i and j = the row of a neighbour of i, both eligible, |(ni.x nj.x + ni.y nj.y) + ni.z nj.z| >=
 *              cos_min and |n . (mj - mi)| <= max_offset for n = ni and n = nj (n the eigenvector of lambda0, m the
 *              mean; the difference rounded once per component, dot products summed as above);
 *   label      (rows,) the segment of a row - the connected components over the eligible rows, numbered in ascending
 *              smallest row - or -1 for a row that is not eligible;
 *   segments   root = node id of the smallest row, n_leaves, and count, mean, cov6 (xx xy xz yy yz zz), eigval,
 *              eigvec (as octl_forest_leaf_stats orders and orients them) merged from the rows' own count, mean and
 *              covariance about the mean of the smallest row; a segment of one leaf copies its row's bits.
 * cos_min = cos(max_angle) is formed by the caller, once.  Size query and fill as octl_forest_pooled_leaf_stats: the
 * call computes what is missing, caches it on the forest with its arguments (dropped wherever the pooled table is),
 * writes *n_rows and *n_segments, and downloads the tables whose pointer is not NULL only when cap_rows >= *n_rows and
 * cap_segments >= *n_segments.  A call with the same arguments on an unchanged forest launches nothing.
 * OCTL_E_INVALID: min_points < 1, cos_min outside [0, 1], max_offset negative or not finite, max_variance NaN, a
 * selection of the wrong length.  OCTL_E_STATE: before the first build.  No reference counterpart.               */
int octl_forest_plane_segments(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int32_t min_points,
                               double max_variance, double cos_min, double max_offset, int64_t cap_rows,
                               int64_t cap_segments, int32_t* neighbour, int32_t* label, int32_t* root,
                               int32_t* n_leaves, int64_t* count, double* mean, double* cov6, double* eigval,
                               double* eigvec, int64_t* n_rows, int64_t* n_segments);
/* The point-to-plane normal equations of a scan against the pooled leaf planes, for ONE rigid transform: what a
 * Gauss-Newton step of scan-to-map registration needs from the device (the 6x6 solve and the iteration are the
 * caller's; octreelib_amd/registration.py has them and the NumPy definition of every number below).  T = row-major
 * 3x4 (R | t), origin = c.  Per query q: p_i = ((R_i0 q_x + R_i1 q_y) + R_i2 q_z) + t_i with every product and sum
 * rounded to f64 (no fma); node, row and r = residual of p exactly as octl_forest_point_to_plane answers them (same
 * state rules and OCTL_E_STATE messages); the point is USED iff row >= 0, r is finite and (max_distance < 0 or |r| <=
 * max_distance).  With d = p - c, J = [d x n, n] (the derivative of r under p <- Rot(w)(p - c) + c + v, xi = (w, v))
 * and the weight w = 1, or for huber_delta > 0: 1 if |r| <= delta else delta / |r|:
 *   sys[0..21)  = upper triangle of H = sum w J J^T, row-major (00, 01, ..., 05, 11, ...),
 *   sys[21..27) = g = sum w J r,  sys[27] = cost = sum rho(r), rho = r^2 / 2 or delta (|r| - delta / 2) beyond delta,
 *   counts[0] = used points, counts[1] = located points (node >= 0).
 * Unused points are skipped (a NaN or inf query never reaches a sum).  node / row / residual: all three NULL, or all
 * three given and then written for every query.  The sums are reduced in a fixed tree that depends on n alone (chunks
 * of 4096 queries; no floating-point atomics): the same call gives the same bits on any device and in either form.
 * With eps = 2^-53 and D = 34 + ceil(ceil(n / 4096) / 256) every entry is within (D + 8) eps sum |term| of the exact
 * sum of the terms formed from p, r and the table's plane bits.  n = 0: no launch, sys = +0.0, counts = 0.
 * OCTL_E_INVALID: n >= 2^31, a NULL pointer, a non-finite T or origin (checked before anything runs).  Two kernels;
 * the host form adds one upload, the downloads and one wait.  Read-only.  No reference counterpart.                 */
int octl_forest_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                    const double origin[3], int32_t min_points, double max_variance,
                                    double max_distance, double huber_delta, double sys[28], int64_t counts[2],
                                    int32_t* node, int32_t* row, double* residual);
/* The same with pointers from octl_dev_alloc (T and origin stay host arrays); no host wait.  n = 0: sys_dev and
 * counts_dev are zeroed by two fills.  No reference counterpart.                                                    */
int octl_forest_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n, const double T[12],
                                           const double origin[3], int32_t min_points, double max_variance,
                                           double max_distance, double huber_delta, double* sys_dev,
                                           int64_t* counts_dev, int32_t* node_dev, int32_t* row_dev,
                                           double* residual_dev);
/* The point-to-point normal equations of a scan against the NEAREST STORED POINT of every transformed query, for ONE
 * rigid transform: classic ICP where the map has no accepted plane to offer (octreelib_amd/registration.py:
 * point_registration_system_np is the definition of every number below).  T, origin = c and p as above.  Per query:
 * the stored point m of the poses of slot_sel / n_sel (NULL: all) nearest to p within max_distance, exactly as
 * octl_forest_nearest answers it for k = 1 (same search, same d2 bits, same total order (d2, slot, index), same state
 * rules); the point is USED iff there is one.  e = fl(p - m) per component, d = p - c, J = [-[d]x, I3] (the derivative
 * of e under p <- Rot(w)(p - c) + c + v), w = 1, or for huber_delta > 0 decided on d2: 1 if d2 <= fl(delta delta) else
 * delta / sqrt(d2):
 *   sys[0..21)  = upper triangle of H = sum w J^T J, row-major: H_ww = sum w (|d|^2 I - d d^T), H_wv = [sum w d]x,
 *                 H_vv = (sum w) I - 17 distinct sums, the rest copies, sign changes and +0.0,
 *   sys[21..27) = g = (sum w d x e, sum w e),  sys[27] = cost = sum rho, rho = d2 / 2 or delta (sqrt(d2) - delta / 2),
 *   counts[0] = used points, counts[1] = queries whose p is finite.
 * slot / index / distance2: all three NULL, or all three given and then written for every query (-1, -1, +inf where
 * nothing lies within max_distance).  The sums are reduced in the tree of octl_forest_registration_system (a function
 * of n alone): the same call gives the same bits on any device and in either form.  With eps = 2^-53 and D as above
 * every entry is within (D + 8) eps sum |term| of the exact sum (csrc/reg_point_term.h fixes the operation order and
 * counts the roundings).  n = 0: no launch, sys = +0.0, counts = 0.  OCTL_E_INVALID: what octl_forest_nearest refuses
 * (max_distance not finite or <= 0 or above twice the voxel edge), n >= 2^31, a NULL pointer, a subset of the three
 * per-point pointers, a non-finite T or origin; OCTL_E_STATE: before build, after map_leaf_points moved rows outside
 * their leaves - all before anything runs.  Three kernels (the block index of the selection is made first when it is
 * missing or stale); the host form adds one upload, the 240-byte download and one wait.  Read-only.  No reference
 * counterpart.                                                                                                        */
int octl_forest_point_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                          const double origin[3], double max_distance, double huber_delta,
                                          const uint8_t* slot_sel, int32_t n_sel, double sys[28], int64_t counts[2],
                                          int32_t* slot, int64_t* index, double* distance2);
/* The same with pointers from octl_dev_alloc (T, origin and slot_sel stay host arrays); no host wait.  n = 0: sys_dev
 * and counts_dev are zeroed by two fills.  No reference counterpart.                                                 */
int octl_forest_point_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n, const double T[12],
                                                 const double origin[3], double max_distance, double huber_delta,
                                                 const uint8_t* slot_sel, int32_t n_sel, double* sys_dev,
                                                 int64_t* counts_dev, int32_t* slot_dev, int64_t* index_dev,
                                                 double* distance2_dev);
/* The nearest-point-to-plane normal equations of a scan, for ONE rigid transform: the correspondence of
 * octl_forest_point_registration_system, the residual of octl_forest_registration_system - what LiDAR odometry uses
 * (octreelib_amd/registration.py: nearest_plane_registration_system_np is the definition of every number below).  T,
 * origin = c and p as above.  Per query: the stored point m of the poses of slot_sel / n_sel (NULL: all) nearest to p
 * within max_distance, exactly as octl_forest_nearest answers it for k = 1; node = the scheme leaf m lies in (as
 * octl_forest_locate answers it for m; -1 without a match) - NOT the leaf of p; row and r = the residual of p against
 * the pooled plane of `node` under the gates min_points / max_variance, as octl_forest_point_to_plane forms them for a
 * point of that leaf (row -1 and r NaN where the leaf has no accepted plane).  The point is USED iff row >= 0 and r is
 * finite; J, the Huber weight on |r| and the 28 sums are those of octl_forest_registration_system (csrc/
 * reg_plane_term.h is the code of both); counts[0] = used points, counts[1] = queries with a correspondence (node >=
 * 0).  max_distance is the search radius alone: there is no gate on |r|.  slot / index / distance2 / node / row /
 * residual: all six NULL, or all six given and then written for every query (-1, -1, +inf, -1, -1, NaN where nothing
 * lies within max_distance).  The sums are reduced in the tree of octl_forest_registration_system (a function of n
 * alone), with its bound.  n = 0: no launch, sys = +0.0, counts = 0.  Refused before anything runs, the forest as it
 * was: what octl_forest_nearest refuses, in its order (OCTL_E_STATE before build; OCTL_E_INVALID for n >= 2^31, a NULL
 * pointer, a subset of the six per-point pointers, a max_distance that is not finite and positive or above twice the
 * voxel edge, a selection of the wrong length; OCTL_E_STATE after map_leaf_points moved rows outside their leaves);
 * OCTL_E_INVALID for a non-finite T or origin; OCTL_E_STATE when the pooled leaf planes are missing or stale, or were
 * made for another pose selection than slot_sel (planes and points must come from the same poses: call
 * octl_forest_pooled_leaf_stats with this selection first).  Three kernels (the block index of the selection is made
 * first when it is missing or stale); the host form adds one upload, the 240-byte download and one wait.  Read-only.
 * No reference counterpart.                                                                                          */
int octl_forest_nearest_plane_registration_system(octl_forest* f, const double* xyz, int64_t n, const double T[12],
                                                  const double origin[3], double max_distance, double huber_delta,
                                                  const uint8_t* slot_sel, int32_t n_sel, int32_t min_points,
                                                  double max_variance, double sys[28], int64_t counts[2],
                                                  int32_t* slot, int64_t* index, double* distance2, int32_t* node,
                                                  int32_t* row, double* residual);
/* The same with pointers from octl_dev_alloc (T, origin and slot_sel stay host arrays); no host wait.  n = 0: sys_dev
 * and counts_dev are zeroed by two fills.  No reference counterpart.                                                 */
int octl_forest_nearest_plane_registration_system_device(octl_forest* f, const double* xyz_dev, int64_t n,
                                                         const double T[12], const double origin[3],
                                                         double max_distance, double huber_delta,
                                                         const uint8_t* slot_sel, int32_t n_sel, int32_t min_points,
                                                         double max_variance, double* sys_dev, int64_t* counts_dev,
                                                         int32_t* slot_dev, int64_t* index_dev, double* distance2_dev,
                                                         int32_t* node_dev, int32_t* row_dev, double* residual_dev);
/* Multi-pose plane adjustment: for ONE rigid transform PER selected pose, the point-to-plane normal equations of every
 * pose against the leaf planes pooled at those transforms - what one block-Jacobi iteration of a sliding-window plane
 * adjustment needs from the device (the 6x6 solves and the iteration are the caller's; octreelib_amd/adjustment.py has
 * them and the NumPy definition of every number below).  slot_sel / n_sel select the poses as
 * octl_forest_pooled_leaf_stats takes them (NULL: all); S = number of selected poses, in ascending slot order;
 * transforms = S row-major 3x4 (R | t), increments applied to the points as they were inserted (leaf membership stays
 * what the last build made it); origin = c.  Per selected (leaf, pose) block, anchor a = the leaf's centre: n, s = sum d,
 * M = sum d d^T, d = x - a, by the chunked wave reduction of octl_forest_pooled_leaf_stats (80 bytes per block, made
 * once per map and selection and kept until a call changes the forest's contents or scheme - the list of
 * octl_forest_pooled_leaf_stats - or the selection is another one).  Per call no point is read: the moments move in
 * closed form, a' = ((R_i0 a_x + R_i1 a_y) + R_i2 a_z) + t_i (rounded f64, no fma), delta = a' - a, s'' = R s + n delta,
 * M'' = R M R^T + delta (R s)^T + (R s) delta^T + n delta delta^T; a leaf pools its blocks in ascending slot order,
 * mean = a + S / N, covariance, eigen-decomposition and sign rule of octl_forest_pooled_leaf_stats (at identity
 * transforms: its bits), plane normal = the smallest eigenvalue's vector.  A leaf is USED iff N >= min_points, at least
 * min_poses of its selected blocks are non-empty, lambda0 is finite and (max_variance < 0 or lambda0 <= max_variance).
 * With r = normal . (x - mean) and J = [(x - c) x normal, normal] over the points x of pose p in used leaves:
 *   sums[p][0..21)  = upper triangle of H_p = sum J J^T, row-major,  sums[p][21..27) = g_p = sum J r,
 *   sums[p][27] = cost_p = sum r^2 / 2,  counts[p][0] = those points,  counts[p][1] = the pose's blocks in used leaves,
 *   n_leaves[0] = leaves pooled, n_leaves[1] = leaves used.
 * Blocks of unused leaves are skipped, never multiplied by zero.  The sums of a pose are reduced in a fixed tree that
 * depends on that pose's selected-block count nb alone (chunks of 1024 blocks; no floating-point atomics): with eps =
 * 2^-53 and D = 22 + ceil(ceil(nb / 1024) / 256) every entry is within (D + 32) eps sum |term| of the exact sum of the
 * block terms formed from the block moments and the leaf table's plane bits, |term| taken product by product
 * (DESIGN.md 4.10).  Three kernels and one host wait on a prepared forest; nothing to reduce (no selected block): no
 * launch, sums = +0.0, counts = 0.  OCTL_E_STATE before the first build; OCTL_E_INVALID: n_sel is not the number of
 * poses, a NULL pointer, a non-finite transform or origin (checked before anything runs).  Read-only apart from its
 * own tables.  No reference counterpart: the reference has no adjustment.                                           */
int octl_forest_adjustment_system(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, const double* transforms,
                                  const double origin[3], int32_t min_points, int32_t min_poses, double max_variance,
                                  double* sums, int64_t* counts, int64_t n_leaves[2]);
/* The tables behind the last octl_forest_adjustment_system call (OCTL_E_STATE if there is none on the forest as it is
 * now).  Leaves, in ascending node id: node, count (pooled points), mean (3), normal (3), lambda0, used (u8);
 * *n_leaves = their number, rows are written only when cap_leaves >= *n_leaves (size query: cap_leaves = 0).  Blocks,
 * in (node, slot) order: blk_node, blk_slot, blk_moments (10 f64 per block: n, sum d (3), sum d d^T xx xy xz yy yz zz
 * about the leaf's centre, at the inserted positions - they do not depend on any transform); *n_blocks, cap_blocks
 * likewise.  Any output may be NULL.  One host wait.  No reference counterpart.                                     */
int octl_forest_adjustment_tables(octl_forest* f, int64_t cap_leaves, int32_t* node, int64_t* count, double* mean,
                                  double* normal, double* lambda0, uint8_t* used, int64_t* n_leaves,
                                  int64_t cap_blocks, int32_t* blk_node, int32_t* blk_slot, double* blk_moments,
                                  int64_t* n_blocks);
/* Write adjusted poses back into the map: one rigid transform per selected pose, applied in place to the rows of the
 * point store, on the device.  slot_sel / n_sel select the poses as octl_forest_adjustment_system takes them (NULL:
 * all); S = number of selected poses, in ascending slot order; transforms = S row-major 3x4 (R | t) - the transforms
 * octl_forest_adjustment_system was evaluated at can be passed straight in.  Every alive row p of a selected pose
 * becomes p'_i = ((R_i0 x + R_i1 y) + R_i2 z) + t_i in f64, every product and sum rounded, no fma
 * (octreelib_amd/registration.py: transform_np, bit for bit).  Rows of the other poses are COPIED bit for bit, not
 * multiplied by an identity (1 * -0.0 + 0 * y is +0.0); a selected pose given the identity does follow the formula.
 * Rows that a mask or filter removed stay removed and keep their place; their coordinates are unspecified afterwards.
 * After a successful call the forest is what a fresh forest of the same configuration would be after the poses had been
 * added again in slot order, each with its surviving rows as moved - no scheme, the voxels the moved points fall into,
 * every derived table stale, the next build starts from the top-level voxels - except that rows keep their positions in
 * the store, so octl_forest_get_perm and octl_forest_nearest still name rows of the clouds as they were first added.
 * TRANSACTIONAL: when an alive moved coordinate is not finite or has a top-level voxel index outside +-2^30 (mode 0),
 * or fails the cube's placement test 0 <= fl(p - corner) < edge (mode 1), the call returns OCTL_E_DOMAIN and nothing
 * observable has changed: the forest is still built and every query answers as before.  A caller's buffer the store
 * reads in place (octl_forest_add_pose_adopt) is never written; after a successful call the store is the forest's own.
 * One upload, one kernel (a stream over the whole store: 24 B read and written per row, plus the alive flag) and one
 * host wait, whatever the size; the moved rows are written out of place into the bucket build's partition scratch,
 * which then swaps with the store (no memory beyond what a build holds).  Works built or not.  S = 0 or an empty store:
 * a successful no-op that changes no state.  OCTL_E_INVALID: n_sel is not the number of poses, NULL transforms with
 * S > 0, a non-finite transform entry (checked before anything runs).  No reference counterpart.                    */
int octl_forest_transform_poses(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, const double* transforms);
/* Let go of poses: the selected poses (slot_sel / n_sel as above; NULL: every pose) leave the map, on the device, and
 * their rows leave the point store.  Afterwards the forest is the forest as it was with those poses absent:
 *  - the scheme stays (node table, voxels, voxel origin, epochs), as after octl_forest_carve: voxels and leaves that
 *    only a removed pose populated stay, empty; ray evidence taken on the scheme is still valid;
 *  - the poses that stay are renumbered densely in ascending order - new_slot (n_sel int32, may be NULL) receives the
 *    new slot of every old one, -1 for a removed pose - and keep every row, alive or dead, at its index within the
 *    pose (octl_forest_get_perm minus the pose's offset, octl_forest_nearest's index), bit for bit;
 *  - every map query over "every pose" answers what it answered over the selection of the remaining poses before;
 *  - the store holds the remaining poses' rows alone (octl_forest_store_size), and the voxel box on the device is
 *    folded again from the alive rows that stay: the next fresh build forms its key geometry from that box.
 * *n_removed (may be NULL): the alive rows of the removed poses.  A built forest loses the removed poses' (leaf, pose)
 * blocks in ONE compaction, which also applies a pending RANSAC mask (as octl_forest_carve and
 * octl_forest_filter_count do); a forest without tables (never built, or reset by octl_forest_transform_poses) takes
 * the store pass alone.  The store pass is out of place, into the block octl_forest_transform_poses writes; a caller's
 * buffer the store reads in place (octl_forest_add_pose_adopt) is never written, and the store is the forest's own
 * afterwards.  Every buffer is reserved before anything changes: OCTL_E_NOMEM leaves the forest as it was.
 * Launches and host waits do not depend on the number of points (the compaction in its fused form): a built forest
 * 4 launches and 2 host waits, a forest without tables 2 launches and 1 host wait; with no pose left the store pass is
 * not launched.  Nothing selected: a successful no-op, no launch, no state change (new_slot: the identity).  Every pose
 * selected: an empty store, the scheme standing.  OCTL_E_INVALID: n_sel is not the number of poses.  OCTL_E_STATE: a
 * built forest to which points were added since (build first).  No reference counterpart.                          */
int octl_forest_remove_poses(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int32_t* new_slot,
                             int64_t* n_removed);
/* Rows the point store holds (alive or not), alive rows among them, poses.  Any output may be NULL. */
int octl_forest_store_size(octl_forest* f, int64_t* n_store, int64_t* n_alive, int32_t* n_poses);
/* Prune the scheme: top-level voxels that hold no point any more leave the voxel list with their whole subtree, and an
 * internal node below which no point is left becomes a leaf (first_child -1, epoch 0); an internal node that stays keeps
 * all eight children, empty ones included.  Nodes are renumbered by a stable compaction - roots stay the nodes
 * [0, voxels_after) in voxel order, levels stay ranges, children stay consecutive; corner, edge, depth and the epochs of
 * the nodes that stay internal keep their bits - and the block table's node column follows.  Points, their order, the
 * store, the alive flags and a pending RANSAC mask are not touched (blocks a pending mask will empty still count as
 * occupied: apply the mask first).  Nothing calls this implicitly.
 * node_map (the first nodes_before of cap_nodes int32, may be NULL): the new id of the node whose cube contains the old
 * node's cube - itself or the collapsed node it vanished into - -1 where the voxel is gone.  old_node (the first
 * nodes_after of cap_nodes int32, may be NULL): new id -> old id.  OCTL_E_INVALID before anything changes when either
 * is given and cap_nodes < nodes_before.  Every buffer is reserved before anything changes: OCTL_E_NOMEM leaves the
 * forest as it was.  Launches and host waits do not depend on the number of points, nodes or levels: one fill, three
 * kernels and ONE host wait find what goes; when nothing does the call ends there and has written no table.  Otherwise
 * two more kernels follow (the node table out of place, then the blocks' node column) without a wait; asking for
 * node_map / old_node costs a second wait, for their download.  A forest without tables (never built, or reset by
 * octl_forest_transform_poses): zeros, no launch.  OCTL_E_STATE: a built forest to which points were added since
 * (build first).  The split statistics of a planar build are dropped.  No reference counterpart.                  */
typedef struct {
  int64_t nodes_before, nodes_after, voxels_before, voxels_after, internal_after, collapsed;
} octl_prune_info;
int octl_forest_prune(octl_forest* f, int64_t cap_nodes, int32_t* node_map, int32_t* old_node, octl_prune_info* info);
/* The eigensolver alone, for tests: n symmetric matrices given as 6 upper-triangle values each. */
int octl_debug_sym3_eigen(octl_ctx* ctx, const double* cov6, int64_t n, double* eigval, double* eigvec);

/* ---- RANSAC on the forest (device resident) ------------------------------------------- */

/* Per-leaf RANSAC plane fit over the blocks listed in block_order (indices into the block
 * table, in the order the reference would concatenate them: grid.py:173-191) — the list is
 * one "batch"; virtual start indices are the running sum of the block sizes in that order
 * (cuda_ransac.py:64-66) and enter the sampling arithmetic exactly as in the reference
 * (cuda_ransac.py:103-107).  hypotheses: (H,k) f64 table (cuda_ransac.py:39-41), H <= 1024.
 * Outputs (any may be NULL), all indexed like block_order: plane (nb,4) f32, best_count
 * (nb) i32, best_index (nb) i32 (lowest hypothesis index attaining the maximum; the
 * reference lets any tied hypothesis win, cuda_ransac.py:140-145).  The inlier mask stays
 * on the device (octl_forest_get_mask / octl_forest_apply_mask).                           */
int octl_forest_ransac(octl_forest* f, const int32_t* block_order, int64_t nb,
                       const double* hypotheses, int32_t H, int32_t k, double threshold,
                       float* plane, int32_t* best_count, int32_t* best_index);
/* All non-empty (leaf, pose) blocks in the order in which the reference lists them: pose
 * slot major, then top-level voxel (lexicographic), then the octree's cached-leaf list
 * (octree_base.py:152-158, octree.py:183-191,256-263), computed on the device.  e0[slot]
 * (nullable = 0) is the build epoch at which the pose's octrees were created: the cached
 * list is history dependent (a pose inserted after a subdivide inherits the whole scheme at
 * once, octree_manager.py:161-171).  order (n_blocks) i32 = indices into the block table.   */
int octl_forest_reference_order(octl_forest* f, const int32_t* e0, int32_t n_e0, int64_t cap,
                                int32_t* order, int64_t* n_blocks);
/* RANSAC over ALL blocks in that order, one reference "batch" per poses_per_batch consecutive
 * slots (grid.py:126,149-157,194); order, virtual starts and the kernel all stay on the device,
 * nothing but the (H,k) table crosses PCIe.  The async launches are NOT synchronised: follow
 * with octl_ctx_sync / get_mask / apply_mask.                                               */
int octl_forest_ransac_all(octl_forest* f, int32_t poses_per_batch, const int32_t* e0,
                           int32_t n_e0, const double* hypotheses, int32_t H, int32_t k,
                           double threshold);
/* Inlier mask of the last ransac call(s), uint8 per storage position.                      */
int octl_forest_get_mask(octl_forest* f, int64_t cap, uint8_t* mask, int64_t* n);
/* Drop the points whose mask byte is 0 from the blocks that were evaluated (apply_mask,
 * octree.py:137-142): compacts the leaf-ordered arrays, updates the block table and marks
 * the points dead for later builds.  Returns the surviving point count - as soon as the count has reached the
 * host: the compaction kernel may still be running (it reads the forest's own arrays only, never a cloud that
 * was taken in place; work enqueued on the context later runs behind it).  octl_ctx_sync waits for it.        */
int octl_forest_apply_mask(octl_forest* f, int64_t* n_alive);
/* The same without waiting for the count (round 6): the kernels are enqueued and the call returns; the surviving
 * point and block counts are booked by the next call that looks at the forest (every octl_forest_* entry point does
 * so first; octl_forest_clear / _destroy drop them unread).  Grid.map_leaf_points_cuda_ransac returns nothing
 * (grid/grid.py:124-215), so a scan loop - insert, subdivide, RANSAC, apply_mask, clear - never waits for this count
 * at all and the next scan's first kernels queue up behind this one's last.  One compaction per context can be in
 * flight: a second one (any forest of the context) books the first before it starts.  A RANSAC launch that met a
 * block larger than it was promised is reported by the next wait of the context, whichever call that is.        */
int octl_forest_apply_mask_async(octl_forest* f);
/* Book the counts of an octl_forest_apply_mask_async now (a no-op otherwise); *n_alive (nullable): surviving points. */
int octl_forest_settle(octl_forest* f, int64_t* n_alive);
/* OctreeNode.filter (octree/octree.py:102-112) for point-count predicates, on the device: every leaf of
 * the poses with slot_sel[slot] != 0 whose point count is outside [lo, hi] is emptied (its points
 * leave the tree), followed by the same compaction as apply_mask.  A criterion `len(points) >= c` is
 * [c, INT64_MAX], `len(points) < c` is [0, c-1], several criteria intersect; lo > hi empties every
 * leaf of the selected poses.  A forest that still holds an unapplied RANSAC mask (octl_forest_ransac
 * without octl_forest_apply_mask*) keeps it: the filter clears the bytes of the leaves it empties in
 * that mask and ONE compaction applies both - the points the RANSAC mask dropped leave as well, also
 * from poses the filter did not select.  The sizes the filter compares are those of the block table
 * before the call (points the pending mask is about to drop still count).                       */
int octl_forest_filter_count(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int64_t lo,
                             int64_t hi, int64_t* n_alive);
/* Drop points by an explicit host mask over storage positions (filter / map_leaf_points
 * paths of the Python layer for arbitrary callables): n = the forest's point count, one byte per
 * position; a byte of 0 drops the point, ANY other value keeps it (as octl_forest_apply_mask).  */
int octl_forest_apply_host_mask(octl_forest* f, const uint8_t* mask, int64_t n,
                                int64_t* n_alive);

/* ---- the reference's operator, stand-alone ------------------------------------------- */

/* CudaRansac(threshold, H, k).evaluate(point_cloud, block_sizes) -> mask
 * (ransac/cuda_ransac.py:43-81).  point_cloud (M,3) f64 leaf-major, block_sizes (B) i32,
 * hypotheses (H,k) f64.  mask_out (M) uint8.  Extensions (nullable): planes_out (B,4) f32,
 * best_count_out (B) i32, best_index_out (B) i32.                                          */
int octl_ransac_evaluate(octl_ctx* ctx, const double* point_cloud, int64_t M,
                         const int32_t* block_sizes, int64_t B, const double* hypotheses,
                         int32_t H, int32_t k, double threshold, uint8_t* mask_out,
                         float* planes_out, int32_t* best_count_out, int32_t* best_index_out);

/* ---- multi-GPU: shard the grid by top-level voxel, route points to their owner --------- */

/* Owner rank of a top-level voxel (pure function, also used by the CPU tests).             */
int32_t octl_voxel_owner(int64_t qx, int64_t qy, int64_t qz, int32_t n_ranks);
#define OCTL_UNIQUE_ID_BYTES 128
/* rank 0 creates the RCCL unique id; the caller distributes the bytes to all ranks.        */
int octl_comm_unique_id(uint8_t id[OCTL_UNIQUE_ID_BYTES]);
int octl_comm_init(octl_ctx* ctx, int32_t n_ranks, int32_t rank,
                   const uint8_t id[OCTL_UNIQUE_ID_BYTES]);
int octl_comm_destroy(octl_ctx* ctx);
/* Route a device-resident cloud (n,3) f64 with global indices gidx (n) i64 (may be NULL:
 * then index_base + i) to the ranks that own the points' top-level voxels (edge L, grid
 * corner c): key + count per destination, 8x8 count exchange, one grouped ncclSend/ncclRecv
 * all-to-all over xGMI.  The received cloud stays on the device inside ctx; its size is
 * returned through *n_recv and it is handed to a forest with octl_forest_add_pose_routed:
 * an empty forest takes the receive buffer over (its own store buffer goes to the router in
 * exchange, no copy), a forest that holds poses already copies the cloud behind them.  Either
 * way the routed cloud is consumed: route again before the next add_pose_routed.             */
int octl_route_points(octl_ctx* ctx, const double* xyz_dev, const int64_t* gidx_dev,
                      int64_t n, int64_t index_base, const double corner[3], double L,
                      int64_t* n_recv, int64_t* send_counts /* [n_ranks], nullable */);
int octl_forest_add_pose_routed(octl_forest* f, int32_t* slot);
/* The same with the routed cloud of ANOTHER context on the same device: routing (its kernels, the
 * RCCL communicator and its stream) can then run in a second context - from a second host thread -
 * while this forest's context builds and fits the previous cloud.  route_ctx may route the next
 * cloud as soon as this call has returned (a buffer swap in the common case; when the cloud has to
 * be copied the call waits for the copy).                                                        */
int octl_forest_add_pose_routed_from(octl_forest* f, octl_ctx* route_ctx, int32_t* slot);
/* global indices of the routed cloud of the last octl_route_points call (n_recv) i64        */
int octl_route_get_gidx(octl_ctx* ctx, int64_t cap, int64_t* gidx, int64_t* n);
/* Number of times the library has made the host wait for the device (stream / event synchronisations)
 * since it was loaded: bench.py reports the round trips per step from it.                        */
int octl_debug_host_syncs(uint64_t* count);
/* Kernel launches + asynchronous fills enqueued by the library so far (process-wide), the companion of
 * octl_debug_host_syncs: bench.py reports launches per step.                                          */
int octl_debug_launches(uint64_t* count);
/* Speculative launches of the bucket build's last kernel (k_bucket_finish enqueued before the host has seen the
 * build's totals, its tables sized from the context's previous build) that did the work / that the host had to
 * repeat the ordinary way (process-wide).  No reference counterpart: the reference has no device queue.        */
int octl_debug_spec_finish(uint64_t* held, uint64_t* missed);
/* Builds whose partition front ran on the context's ahead stream, next to the previous scan's RANSAC and mask
 * (octl_forest_build: Streams; process-wide).  No reference counterpart: the reference has no device queue.   */
int octl_debug_builds_ahead(uint64_t* count);

/* Test hook: the communicator-independent half of octl_route_points for ANY number of ranks -
 * destination of every point (host cloud in), per-destination counts [n_ranks], and the packed
 * send buffers (points and global indices stably partitioned by destination).                */
int octl_debug_route_partition(octl_ctx* ctx, const double* xyz, int64_t n, int64_t index_base,
                               double L, int32_t n_ranks, int64_t* counts, double* xyz_out,
                               int64_t* gidx_out);
/* sum-all-reduce of small int64 vectors (counters) over the communicator                   */
int octl_comm_allreduce_i64(octl_ctx* ctx, int64_t* inout_host, int32_t n);

/* ---- small device utilities used by bench.py (inputs resident in HBM) ------------------ */
int octl_dev_alloc(octl_ctx* ctx, int64_t bytes, void** dptr);
int octl_dev_free(octl_ctx* ctx, void* dptr);
int octl_dev_upload(octl_ctx* ctx, void* dptr, const void* src, int64_t bytes);
int octl_dev_download(octl_ctx* ctx, void* dst, const void* dptr, int64_t bytes);
/* ---- asynchronous host feed ---------------------------------------------------------------------
 * Replaces the synchronous host-to-device copies of CudaRansac.evaluate (ransac/cuda_ransac.py:57-67) and of
 * Grid.insert_points' storage step for a loop over scans: the upload of scan i+1 runs on a copy stream of
 * its own while the context's compute stream builds and fits scan i.
 *   octl_host_alloc / octl_host_free   page-locked host memory (a copy out of it is a DMA the host does not
 *                                      wait for; out of pageable memory the call blocks while HIP stages it)
 *   octl_dev_upload_async              enqueue the copy host -> dptr behind the compute work enqueued so far;
 *                                      returns at once.  `src` must stay unchanged until octl_ctx_sync_uploads
 *                                      (or octl_dev_free / octl_host_free of either end) has returned.
 *   octl_ctx_sync_uploads              host waits for every upload enqueued so far
 * octl_forest_add_pose_device / octl_forest_add_pose_adopt order the compute stream behind the uploads enqueued
 * before them (on the device; the host does not wait).                                              */
int octl_host_alloc(octl_ctx* ctx, int64_t bytes, void** p);
int octl_host_free(octl_ctx* ctx, void* p);
int octl_dev_upload_async(octl_ctx* ctx, void* dptr, const void* src, int64_t bytes);
int octl_ctx_sync_uploads(octl_ctx* ctx);
/* measured device copy bandwidth (bytes/s) over `bytes`, for the roofline report           */
int octl_dev_copy_bandwidth(octl_ctx* ctx, int64_t bytes, int iters, double* bytes_per_s);

/* Test hook for the allocation-failure paths: the nth growth of a device buffer from now on (every device
 * allocation of the library is one) fails with OCTL_E_NOMEM exactly as a failed hipMalloc does; nth <= 0 disarms.
 * *seen (nullable) receives the number of growths since the hook was last armed, so a test can sweep nth over
 * everything an operation allocates.  Process-wide.                                                     */
int octl_debug_fail_alloc(int64_t nth, int64_t* seen);

/* What the communicator itself reports (ncclCommCount / ncclCommUserRank / ncclGetVersion; -1 where the collective
 * library does not export the query), and the device behind a context (PCI bus id as "dddd:bb:dd.f", the 16-byte
 * UUID of its properties, its compute units): a multi-GPU run prints these so that its line proves what ran where.
 * The reference has no counterpart (no distributed code).                                            */
int octl_comm_info(octl_ctx* ctx, int32_t* n_ranks, int32_t* user_rank, int32_t* version);
int octl_device_identity(octl_ctx* ctx, char pci_bus_id[32], uint8_t uuid[16], int32_t* cus);

/* Diagnostic switches of a context (tests and A/B runs compare code paths: "NO_BUCKET_BUILD", "BUCKET_POINTS",
 * "SYNC_GEOM", "NO_GEOM_HINT", "GEOM_MARGIN", "NO_EXACT_DIGITS", "NO_FAST_ORDER", "NO_BUCKET_HISTORY", "NO_CUBE_FAST",
 * "NO_CUBE_PREFIX", "CUBE_PREFIX_MIN", "NO_INCREMENTAL", "ROUTE_SELF_SENDRECV", "TRACE_BUILD", "SCAN",
 * "NO_FUSED_TABLES", "NO_SPIN_WAIT", "NO_SPEC_FINISH", "RANSAC_WAVES", "NO_RANSAC_PRESCREEN", "NO_BUILD_AHEAD",
 * "BUILD_AHEAD_MIN_POINTS" (the one switch whose unset value is not 0: -1 = the library's bound); an "OCTL_" prefix is
 * accepted; the table in INTEGRATION.md says what each one does).  octl_ctx_create reads OCTL_<NAME> from the
 * environment ONCE, as a number: OCTL_X=0 is OFF (rounds 1-4 tested only for the variable's presence), a value that
 * is not a number is 1, and setting the environment after the context exists has no effect - this call changes a
 * switch of a live context.  0 = the shipped behaviour.  The reference has no counterpart.                       */
int octl_debug_set_option(octl_ctx* ctx, const char* name, int64_t value);

/* The key geometry of a single-pass bucket build as a pure HOST function (no context, no GPU: the same code the
 * device evaluates, csrc/bucket_build.hip: geom_from_box): for a cloud whose true voxel box is tb = {min x, y, z,
 * max x, y, z}, `want` buckets wanted (a power of two), n_alive points, `target` points per bucket and `margin`
 * voxels of slack, it returns the padded box of the linear keys, the bucket width in keys, the bucket count - and
 * *mismatches = the number of keys of that box for which the kernels' division-free bucket index
 * (trunc(fma(key, 1/width, 0.5/width))) differs from key / width (must be 0).  *valid = 0 with the library's reason
 * code when the box is not a single-pass case.  Replaces nothing in the reference, which rebuckets every call from
 * scratch (grid/grid.py:72-90); tests/test_cpu_abi.py drives it.                                              */
int octl_debug_key_geometry(const int32_t tb[6], uint64_t want, int64_t n_alive, uint32_t target, int32_t margin,
                            int32_t bb_out[6], uint32_t* width, uint32_t* n_buckets, int32_t* valid,
                            int64_t* mismatches);

/* ---- test hooks for the device-wide primitives (host in / host out) ----------------------- */
int octl_debug_exclusive_scan(octl_ctx* ctx, const uint32_t* in, int64_t n, uint32_t* out,
                              uint32_t* total);
int octl_debug_radix_sort(octl_ctx* ctx, uint64_t* keys, uint32_t* vals, int64_t n,
                          int key_bits);
/* The plane fit's arithmetic shortcuts (csrc/ransac.hip: div3_by_norm, div_by_small_int,
 * sqrt_rn_guarded) on caller data: q3[i,:] = num3[i,:] / den[i] (den > 0, |num| <= 2^60 den),
 * ck[i] = c[i] / kdiv (1 <= kdiv <= 16), sq[i] = sqrt(c[i]).  All must equal the IEEE f64 results
 * the reference computes (util.py:42-44,76,80-82).                                           */
int octl_debug_plane_arith(octl_ctx* ctx, const double* num3, const double* den, const double* c,
                           int32_t kdiv, int64_t n, double* q3, double* ck, double* sq);
/* The same three operations without their per-lane range guards, as the plane fit runs them on a block whose
 * coordinates are all +0.0 or in [2^-30, 2^31) (the range certificate of csrc/ransac.hip: coord_in_fast_range).  The
 * caller keeps the operands in the certified ranges: den in [2^-200, 2^138], num3 zero or in [2^-552, den],
 * c = +0.0 or |c| in [2^-82, 2^35) for c / kdiv, c in [2^-400, 2^276] for sqrt(c).                  */
int octl_debug_plane_arith_certified(octl_ctx* ctx, const double* num3, const double* den, const double* c,
                                     int32_t kdiv, int64_t n, double* q3, double* ck, double* sq);

#ifdef __cplusplus
}
#endif
#endif /* OCTREELIB_HIP_H */
