// Stand-alone host program for tests/test_cpu_prune_host.py: runs the steps of octl_forest_prune
// (octreelib_amd/csrc/prune_map.h, the code the kernels of prune.hip run, compiled for the CPU) over a node table and a
// block table read from one file and writes the pruned tables to another.  Every array is a heap block of exactly its
// size, so a build with -fsanitize=address,undefined turns an index outside a table into an error.  No GPU, no HIP call.
//
//   prune_host <in> <out> <items per tile>
//   in:  int64 {N, V, B, mode, S}, seg end i64[S], seg depth i64[S],
//        i32[N] each: voxel, depth, parent, first_child, epoch; corner f64[3 N], edge f64[N]; blk_node i32[B]
//   out: int64 {N', V', internal, collapsed, deepest, S}, new seg a i64[S], b i64[S],
//        i32[N'] each: voxel, depth, parent, first_child, epoch, old_id; corner f64[3 N'], edge f64[N'];
//        node_map i32[N], blk_node i32[B], voxel keys u64[V'] (key v of the input is 1000 + v)
// Mark, flags, node pass and block pass run tile by tile as the kernels' workgroups do - the flags' counters through a
// per-tile copy that is flushed like the workgroup's - and the scan is serial.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prune_map.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "prune_host: the input ends early\n");
    exit(2);
  }
  return v;
}

template <typename T>
static void put(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const int64_t tile = atoll(argv[3]);
  const auto h = take<int64_t>(in, 5);
  const int64_t N = h[0], V = h[1], B = h[2];
  const int mode = (int)h[3];
  const int S = (int)h[4];
  if (tile < 1 || N < 0 || V < 0 || V > N || B < 0 || S < 1 || S > PRUNE_MAX_SEGS) return 2;
  const auto seg_end = take<int64_t>(in, (size_t)S), seg_depth = take<int64_t>(in, (size_t)S);
  auto voxel = take<int32_t>(in, (size_t)N), depth = take<int32_t>(in, (size_t)N), parent = take<int32_t>(in, (size_t)N),
       first_child = take<int32_t>(in, (size_t)N), epoch = take<int32_t>(in, (size_t)N);
  auto corner = take<double>(in, (size_t)N * 3), edge = take<double>(in, (size_t)N);
  auto blk_node = take<int32_t>(in, (size_t)B);
  fclose(in);
  if (seg_end[(size_t)S - 1] != N || seg_end[0] != V) return 2;

  PruneSegs segs;
  segs.n = S;
  for (int s = 0; s < S; ++s) segs.end[s] = seg_end[(size_t)s];
  std::vector<uint32_t> start((size_t)N, 7u), count((size_t)N, 8u), scount((size_t)N, 9u);
  std::vector<int32_t> old_id((size_t)N, -1);
  std::vector<uint64_t> vcode((size_t)V);
  for (int64_t v = 0; v < V; ++v) vcode[(size_t)v] = 1000u + (uint64_t)v;

  // 1 + 2: fill, mark
  std::vector<uint32_t> occ((size_t)N, 0u), res((size_t)PRUNE_W_SEG + (size_t)S, 0u);
  for (int64_t b0 = 0; b0 < B; b0 += tile)
    for (int64_t b = b0; b < B && b < b0 + tile; ++b) prune_mark_climb(blk_node[(size_t)b], parent.data(), occ.data());
  // 3: flags, with the counters of one tile flushed behind it
  std::vector<uint32_t> keep((size_t)N), new_id((size_t)N);
  for (int64_t i0 = 0; i0 < N; i0 += tile) {
    std::vector<uint32_t> cnt((size_t)PRUNE_W_SEG + (size_t)S, 0u);
    for (int64_t i = i0; i < N && i < i0 + tile; ++i) {
      const bool k = prune_keep(i, mode, parent.data(), occ.data());
      keep[(size_t)i] = k ? 1u : 0u;
      if (!k) continue;
      cnt[(size_t)(PRUNE_W_SEG + prune_seg_of(segs, i))] += 1u;
      if (i < V) cnt[PRUNE_W_VOXELS] += 1u;
      if (first_child[(size_t)i] >= 0) cnt[occ[(size_t)i] ? PRUNE_W_INTERNAL : PRUNE_W_COLLAPSED] += 1u;
    }
    for (size_t w = 0; w < cnt.size(); ++w) res[w] += cnt[w];
  }
  // 4: scan
  uint32_t run = 0;
  for (int64_t i = 0; i < N; ++i) {
    new_id[(size_t)i] = run;
    run += keep[(size_t)i];
  }
  res[PRUNE_W_TOTAL] = run;
  std::vector<int64_t> seg_a((size_t)S), seg_b((size_t)S);
  const int64_t n_new = prune_rewrite_segs(S, res.data() + PRUNE_W_SEG, seg_a.data(), seg_b.data());
  const int64_t v_new = res[PRUNE_W_VOXELS];
  if (n_new != (int64_t)run || seg_b[0] != v_new) return 3;   // (the counts by level agree with the scan)
  int64_t deepest = 0;
  for (int s = 0; s < S; ++s)
    if (seg_b[(size_t)s] > seg_a[(size_t)s] && seg_depth[(size_t)s] > deepest) deepest = seg_depth[(size_t)s];

  // 5: the node pass, into tables of exactly the new size
  std::vector<uint32_t> start2((size_t)n_new), count2((size_t)n_new), scount2((size_t)n_new);
  std::vector<int32_t> voxel2((size_t)n_new), depth2((size_t)n_new), parent2((size_t)n_new), fc2((size_t)n_new),
      old2((size_t)n_new), epoch2((size_t)n_new), node_map((size_t)N);
  std::vector<double> corner2((size_t)n_new * 3), edge2((size_t)n_new);
  std::vector<uint64_t> vcode2((size_t)v_new);
  const PruneCols src{start.data(), count.data(), scount.data(), depth.data(), voxel.data(), parent.data(),
                      first_child.data(), old_id.data(), epoch.data(), corner.data(), edge.data()};
  const PruneCols dst{start2.data(), count2.data(), scount2.data(), depth2.data(), voxel2.data(), parent2.data(),
                      fc2.data(), old2.data(), epoch2.data(), corner2.data(), edge2.data()};
  for (int64_t i0 = 0; i0 < N; i0 += tile)
    for (int64_t i = i0; i < N && i < i0 + tile; ++i)
      prune_write_node(i, src, dst, occ.data(), keep.data(), new_id.data(), V, vcode.data(), vcode2.data(),
                       node_map.data());
  for (int64_t y = 0; y < n_new; ++y)
    if (start2[(size_t)y] != 7u || count2[(size_t)y] != 8u || scount2[(size_t)y] != 9u) return 3;
  // 6: the block pass
  for (int64_t b0 = 0; b0 < B; b0 += tile)
    for (int64_t b = b0; b < B && b < b0 + tile; ++b) blk_node[(size_t)b] = node_map[(size_t)blk_node[(size_t)b]];

  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  const int64_t head[6] = {n_new, v_new, (int64_t)res[PRUNE_W_INTERNAL], (int64_t)res[PRUNE_W_COLLAPSED], deepest, S};
  fwrite(head, 8, 6, out);
  put(out, seg_a);
  put(out, seg_b);
  put(out, voxel2);
  put(out, depth2);
  put(out, parent2);
  put(out, fc2);
  put(out, epoch2);
  put(out, old2);
  put(out, corner2);
  put(out, edge2);
  put(out, node_map);
  put(out, blk_node);
  put(out, vcode2);
  return fclose(out) == 0 ? 0 : 2;
}
