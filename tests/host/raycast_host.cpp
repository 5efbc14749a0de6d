// Stand-alone host program for tests/test_cpu_raycast_host.py: runs the traversal of octl_forest_raycast
// (octreelib_amd/csrc/raycast_walk.h, the code the kernel runs, compiled for the CPU) over the tables and rays of one
// file and writes the answers to another.  Every table is a heap block of exactly its size, so a build with
// -fsanitize=address,undefined turns a lookup outside a table into an error.  No GPU, no HIP call.
//
//   raycast_host <in> <out>
//   in:  int64 {mode, V, n_nodes, n_rec, n_rows, n_rays, surface, min_points, org x, org y, org z}, double {L,
//        max_variance}, then vcode u64[V], first_child i32[N], parent i32[N], corner f64[3N], edge f64[N],
//        first i32[N], cnt i32[N], rec u32[4 n_rec], node_row i32[N], rows f64[8 n_rows], origins f64[3n],
//        directions f64[3n], t_min f64[n], t_max f64[n]
//   out: node i32[n], row i32[n], t f64[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "raycast_walk.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "raycast_host: the input ends early\n");
    exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const auto h = take<int64_t>(in, 11);
  const auto g = take<double>(in, 2);
  const int64_t V = h[1], N = h[2], n_rec = h[3], n_rows = h[4], n = h[5];
  const auto vcode = take<uint64_t>(in, (size_t)V);
  const auto first_child = take<int32_t>(in, (size_t)N), parent = take<int32_t>(in, (size_t)N);
  const auto corner = take<double>(in, (size_t)N * 3), edge = take<double>(in, (size_t)N);
  const auto first = take<int32_t>(in, (size_t)N), cnt = take<int32_t>(in, (size_t)N);
  const auto rec = take<uint4>(in, (size_t)n_rec);
  const auto node_row = take<int32_t>(in, (size_t)N);
  const auto rows = take<double2>(in, (size_t)n_rows * 4);
  const auto org = take<double>(in, (size_t)n * 3), dir = take<double>(in, (size_t)n * 3);
  const auto t_min = take<double>(in, (size_t)n), t_max = take<double>(in, (size_t)n);
  fclose(in);

  RayTables T;
  T.t.mode = (int)h[0];
  T.t.L = g[0];
  T.t.org.x = (int32_t)h[8], T.t.org.y = (int32_t)h[9], T.t.org.z = (int32_t)h[10];
  T.t.vcode = vcode.data();
  T.t.V = V;
  T.t.first_child = first_child.data();
  T.t.corner = corner.data();
  T.t.edge = edge.data();
  T.parent = parent.data();
  T.first = first.data();
  T.cnt = cnt.data();
  T.rec = rec.data();
  T.pt.node_row = node_row.data();
  T.pt.rows = rows.data();
  T.pt.min_points = (int32_t)h[7];
  T.pt.max_variance = g[1] >= 0.0 ? g[1] : -1.0;
  T.min_points = (int32_t)h[7];
  T.max_steps = 4 * N + 64;

  std::vector<int32_t> node((size_t)n), row((size_t)n);
  std::vector<double> t((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const RayBest b = h[6] == 1 ? ray_cast<true>(T, &org[3 * i], &dir[3 * i], t_min[i], t_max[i])
                                : ray_cast<false>(T, &org[3 * i], &dir[3 * i], t_min[i], t_max[i]);
    node[(size_t)i] = b.node, row[(size_t)i] = b.row, t[(size_t)i] = b.t;
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  fwrite(node.data(), 4, (size_t)n, out);
  fwrite(row.data(), 4, (size_t)n, out);
  fwrite(t.data(), 8, (size_t)n, out);
  return fclose(out) == 0 ? 0 : 2;
}
