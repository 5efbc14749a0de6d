// Stand-alone host program for tests/test_cpu_neighbourhood_host.py: runs the rows of octl_forest_neighbourhood_stats
// and octl_forest_point_stats (octreelib_amd/csrc/radius_moments.h: the sink, finish and the eigen solver, over the walk
// of nearest_walk.h - the code the kernels run, compiled for the CPU) over the tables and queries of one file and writes
// the rows to another.  Every table is a heap block of exactly its size, so a build with -fsanitize=address,undefined
// turns a lookup outside a table into an error.  No GPU, no HIP call.
//
//   moments_host <in> <out>
//   in:  int64 {mode, V, n_nodes, n_rec, n_ord, n, eigen, org x, org y, org z}, double {L, radius}, then vcode u64[V],
//        first_child i32[N], parent i32[N], corner f64[3N], edge f64[N], first i32[N], cnt i32[N], rec u32[4 n_rec],
//        xyz_ord f64[3 n_ord], ord_idx u32[n_ord], queries f64[3n]
//   out: count i64[n], mean f64[3n], cov f64[6n], eigval f64[3n], eigvec f64[9n] (the last two only with eigen != 0)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "radius_moments.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "moments_host: the input ends early\n");
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
  const int64_t V = h[1], N = h[2], n_rec = h[3], n_ord = h[4], n = h[5];
  const bool eigen = h[6] != 0;
  const auto vcode = take<uint64_t>(in, (size_t)V);
  const auto first_child = take<int32_t>(in, (size_t)N), parent = take<int32_t>(in, (size_t)N);
  const auto corner = take<double>(in, (size_t)N * 3), edge = take<double>(in, (size_t)N);
  const auto first = take<int32_t>(in, (size_t)N), cnt = take<int32_t>(in, (size_t)N);
  const auto rec = take<uint4>(in, (size_t)n_rec);
  const auto xyz_ord = take<double>(in, (size_t)n_ord * 3);
  const auto ord_idx = take<uint32_t>(in, (size_t)n_ord);
  const auto q = take<double>(in, (size_t)n * 3);
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
  T.parent = parent.data();
  T.first = first.data();
  T.cnt = cnt.data();
  T.rec = rec.data();
  T.xyz_ord = xyz_ord.data();
  T.ord_idx = ord_idx.data();
  T.max_steps = 4 * N + 64;

  const double r = g[1], r2 = r * r;
  std::vector<int64_t> count((size_t)n);
  std::vector<double> mean((size_t)n * 3), cov((size_t)n * 6), w(eigen ? (size_t)n * 3 : 0), v(eigen ? (size_t)n * 9 : 0);
  for (int64_t i = 0; i < n; ++i)
    count[(size_t)i] = moments_row(T, q[3 * i + 0], q[3 * i + 1], q[3 * i + 2], r, r2, mean.data() + 3 * i,
                                   cov.data() + 6 * i, eigen ? w.data() + 3 * i : nullptr, v.data() + (eigen ? 9 * i : 0));
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  put(out, count), put(out, mean), put(out, cov), put(out, w), put(out, v);
  return fclose(out) == 0 ? 0 : 2;
}
