// octl_forest_prune (prune.hip): which scheme nodes stay when the empty parts of a map are dropped,
// where a node that goes is still contained, and what a row of the new node table holds.  __host__ __device__, so that
// the stand-alone host program tests/host/prune_host.cpp runs the very text of the kernels over heap arrays of exactly
// their size (AddressSanitizer / UBSan; tests/test_cpu_prune_host.py).  query.prune_np is the definition.
//
// occ[n] != 0: some (leaf, pose) block - non-empty by construction - lies in the subtree of n.
//   keep      a root stays iff occ[root] (a single cube, mode 1: always); any other node stays iff occ[parent]: the
//             eight children of a node stay or go together, and the kept set is closed towards the roots.
//   collapse  a kept internal node with !occ becomes a leaf: first_child = -1, epoch = 0.
//   number    new id = exclusive scan of the keep flags (stable): roots stay [0, V') in voxel order, the nodes of a
//             level range stay a range, children stay eight consecutive ids.
//   contain   node_map[old] = new id of the node itself or of the first kept node above it; -1: its voxel is gone.
//
// What one call does, in stream order (prune.hip: octl_forest_prune has the code):
//   1. fill              occ and the counters of step 3 zeroed (one fill)
//   2. k_prune_mark      one lane per block: sets occ[node] and climbs `parent` while it is the lane that flips a flag
//                        0 -> 1 (prune_mark_climb): O(nodes) flips whatever the depth, no sweep by level
//   3. k_prune_flags     one lane per node: the keep flag, and per workgroup the counts the host commits by - kept nodes
//                        of every level range, kept roots, internal nodes that stay internal, nodes that collapse
//   4. scan              new ids; its total is the new node count
//      -- the ONE host wait: the counts.  Nothing to drop or collapse: the call ends here, nothing written --
//   5. k_prune_nodes     one lane per OLD node: a kept one writes its row of the other node table and its voxel key,
//                        every one writes node_map (prune_write_node)
//   6. k_prune_blocks    blk_node through node_map, in place: the first write to anything the forest reads
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PRUNE_HD __host__ __device__ __forceinline__

// level ranges one call can rewrite (two per depth at most: the bucket build's and the level loop's)
#define PRUNE_MAX_SEGS 128
// the words the host waits for: [0] scan total, then the counters k_prune_flags adds into
enum { PRUNE_W_TOTAL = 0, PRUNE_W_VOXELS = 1, PRUNE_W_INTERNAL = 2, PRUNE_W_COLLAPSED = 3, PRUNE_W_SEG = 4,
       PRUNE_WORDS = PRUNE_W_SEG + PRUNE_MAX_SEGS };

// end of every level range, ascending: the ranges tile [0, n_nodes) in this order
struct PruneSegs {
  int64_t end[PRUNE_MAX_SEGS];
  int32_t n;
};

// the columns of a node table (build_common.h: NodePtrs has the same members)
struct PruneCols {
  uint32_t *start, *count, *scount;
  int32_t *depth, *voxel, *parent, *first_child, *old_id, *epoch;
  double *corner, *edge;
};

// set a flag, tell what it was.  On the device an exchange: of the lanes that meet at a node exactly one goes on
PRUNE_HD uint32_t prune_flag_set(uint32_t* flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicExch(flag, 1u);
#else
  const uint32_t was = *flag;
  *flag = 1u;
  return was;
#endif
}

// a block in leaf `node`: every node from it to its root is occupied.  Stops at the first flag that was set already
PRUNE_HD void prune_mark_climb(int32_t node, const int32_t* parent, uint32_t* occ) {
  while (node >= 0 && prune_flag_set(&occ[node]) == 0u) node = parent[node];
}

PRUNE_HD bool prune_keep(int64_t i, int mode, const int32_t* parent, const uint32_t* occ) {
  const int32_t p = parent[i];
  return p < 0 ? (mode == 1 || occ[i] != 0u) : occ[p] != 0u;
}

// a kept node that has children and nothing below them
PRUNE_HD bool prune_collapses(int64_t i, const int32_t* first_child, const uint32_t* occ) {
  return first_child[i] >= 0 && occ[i] == 0u;
}

// the level range of node i: the first whose end lies behind it
PRUNE_HD int prune_seg_of(const PruneSegs& s, int64_t i) {
  int lo = 0, hi = s.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s.end[mid] > i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the kept node that contains node i: itself, or the first kept node above it; -1: none (the voxel goes)
PRUNE_HD int32_t prune_container(int32_t i, const int32_t* parent, const uint32_t* keep) {
  while (i >= 0 && keep[i] == 0u) i = parent[i];
  return i;
}

// One OLD node: its row of the new table and its voxel key when it stays, its entry of node_map always.
// n_voxels: roots are the nodes [0, n_voxels), root v belongs to voxel v.  vcode_in / vcode_out may both be null.
PRUNE_HD void prune_write_node(int64_t i, const PruneCols& src, const PruneCols& dst, const uint32_t* occ,
                               const uint32_t* keep, const uint32_t* new_id, int64_t n_voxels, const uint64_t* vcode_in,
                               uint64_t* vcode_out, int32_t* node_map) {
  if (keep[i] == 0u) {
    const int32_t c = prune_container((int32_t)i, src.parent, keep);
    node_map[i] = c < 0 ? -1 : (int32_t)new_id[c];
    return;
  }
  const int64_t y = new_id[i];
  node_map[i] = (int32_t)y;
  const bool leaf_now = prune_collapses(i, src.first_child, occ);
  const int32_t p = src.parent[i], fc = src.first_child[i];
  dst.start[y] = src.start[i];
  dst.count[y] = src.count[i];
  dst.scount[y] = src.scount[i];
  dst.depth[y] = src.depth[i];
  dst.voxel[y] = (int32_t)new_id[src.voxel[i]];
  dst.parent[y] = p < 0 ? -1 : (int32_t)new_id[p];
  dst.first_child[y] = (fc < 0 || leaf_now) ? -1 : (int32_t)new_id[fc];
  dst.old_id[y] = (int32_t)i;
  dst.epoch[y] = leaf_now ? 0 : src.epoch[i];
  dst.corner[3 * y + 0] = src.corner[3 * i + 0];
  dst.corner[3 * y + 1] = src.corner[3 * i + 1];
  dst.corner[3 * y + 2] = src.corner[3 * i + 2];
  dst.edge[y] = src.edge[i];
  if (i < n_voxels && vcode_out) vcode_out[y] = vcode_in[i];
}

// The level ranges behind the compaction: range s keeps kept[s] of its nodes and the ranges still tile the table in
// the same order, so range s becomes [kept[0] + .. + kept[s - 1], that + kept[s]).  Returns the new node count.
static inline int64_t prune_rewrite_segs(int n, const uint32_t* kept, int64_t* new_a, int64_t* new_b) {
  int64_t run = 0;
  for (int s = 0; s < n; ++s) {
    new_a[s] = run;
    run += (int64_t)kept[s];
    new_b[s] = run;
  }
  return run;
}
