// Stand-alone host program for tests/test_cpu_cluster_host.py: runs the linking sink of octl_forest_cluster_points
// (octreelib_amd/csrc/cluster_link.h over the walk of nearest_walk.h and the union-find of union_find.h - the code the
// kernels run, compiled for the CPU, single-threaded: the host branch of union_find.h uses plain loads and stores) over
// the tables of one file, then finds root, size and smallest id of every position as k_cluster_flatten does, and writes
// them to another.  Every table is a heap block of exactly its size, so a build with -fsanitize=address,undefined turns
// a lookup outside a table into an error.  No GPU, no HIP call.
//
//   cluster_host <in> <out>
//   in:  int64 {mode, V, n_nodes, n_rec, n_ord, reversed, 0, org x, org y, org z}, double {L, radius}, then vcode u64[V],
//        first_child i32[N], parent i32[N], corner f64[3N], edge f64[N], first i32[N], cnt i32[N], rec u32[4 n_rec],
//        xyz_ord f64[3 n_ord], ord_idx u32[n_ord]          (reversed != 0: the positions are linked last to first)
//   out: root i32[n_ord], size u32[n_ord], first u64[n_ord] (slot << 32 | store index - store offset of the record)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cluster_link.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "cluster_host: the input ends early\n");
    exit(2);
  }
  return v;
}

template <typename T>
static void put(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const auto h = take<int64_t>(in, 10);
  const auto g = take<double>(in, 2);
  const int64_t V = h[1], N = h[2], n_rec = h[3], n_ord = h[4];
  const bool reversed = h[5] != 0;
  const auto vcode = take<uint64_t>(in, (size_t)V);
  const auto first_child = take<int32_t>(in, (size_t)N), up = take<int32_t>(in, (size_t)N);
  const auto corner = take<double>(in, (size_t)N * 3), edge = take<double>(in, (size_t)N);
  const auto first = take<int32_t>(in, (size_t)N), cnt = take<int32_t>(in, (size_t)N);
  const auto rec = take<uint4>(in, (size_t)n_rec);
  const auto xyz_ord = take<double>(in, (size_t)n_ord * 3);
  const auto ord_idx = take<uint32_t>(in, (size_t)n_ord);
  fclose(in);

  NNTables T;
  T.t.mode = (int)h[0];
  T.t.L = g[0];
  T.t.org.x = (int32_t)h[7], T.t.org.y = (int32_t)h[8], T.t.org.z = (int32_t)h[9];
  T.t.vcode = vcode.data();
  T.t.V = V;
  T.t.first_child = first_child.data();
  T.t.corner = corner.data();
  T.t.edge = edge.data();
  T.parent = up.data();
  T.first = first.data();
  T.cnt = cnt.data();
  T.rec = rec.data();
  T.xyz_ord = xyz_ord.data();
  T.ord_idx = ord_idx.data();
  T.max_steps = 4 * N + 64;

  // k_cluster_init: a position of a record's block is a vertex
  std::vector<int32_t> parent((size_t)n_ord, -1);
  std::vector<uint64_t> id((size_t)n_ord, ~0ull);
  for (const uint4& r : rec)
    for (uint32_t j = 0; j < r.y; ++j) {
      parent[(size_t)r.x + j] = (int32_t)(r.x + j);
      id[(size_t)r.x + j] = ((uint64_t)r.z << 32) | (uint64_t)(ord_idx[(size_t)r.x + j] - r.w);
    }
  // k_cluster_link
  const double r = g[1], r2 = r * r;
  const int64_t max_steps = 8 * n_ord + 64;
  for (int64_t i = 0; i < n_ord; ++i) {
    const int64_t pos = reversed ? n_ord - 1 - i : i;
    if (parent[(size_t)pos] < 0) continue;
    if (!cluster_link_one(T, parent.data(), (int32_t)pos, r, r2, max_steps)) {
      fprintf(stderr, "cluster_host: the union-find ran out of its step budget at position %lld\n", (long long)pos);
      return 3;
    }
  }
  // k_cluster_flatten
  std::vector<int32_t> root((size_t)n_ord, -1);
  std::vector<uint32_t> size((size_t)n_ord, 0);
  std::vector<uint64_t> smallest((size_t)n_ord, ~0ull);
  for (int64_t pos = 0; pos < n_ord; ++pos) {
    if (parent[(size_t)pos] < 0) continue;
    int64_t budget = max_steps;
    const int32_t rt = uf_find(parent.data(), (int32_t)pos, budget);
    if (rt < 0) return 3;
    root[(size_t)pos] = rt;
    size[(size_t)rt] += 1;
    if (id[(size_t)pos] < smallest[(size_t)rt]) smallest[(size_t)rt] = id[(size_t)pos];
  }
  for (int64_t pos = 0; pos < n_ord; ++pos)
    if (root[(size_t)pos] >= 0) {
      size[(size_t)pos] = size[(size_t)root[(size_t)pos]];
      smallest[(size_t)pos] = smallest[(size_t)root[(size_t)pos]];
    }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  put(out, root), put(out, size), put(out, smallest);
  return fclose(out) == 0 ? 0 : 2;
}
