// Stand-alone host program for tests/test_cpu_evidence_host.py: runs the walk of octl_forest_ray_evidence
// (octreelib_amd/csrc/raycast_walk.h: ray_evidence, the code the kernel runs, compiled for the CPU) over the tables
// and rays of one file and writes the counters to another.  Every table is a heap block of exactly its size, so a
// build with -fsanitize=address,undefined turns a lookup outside a table into an error.  No GPU, no HIP call.
//
//   evidence_host <in> <out>
//   in:  int64 {mode, V, n_nodes, n_rays, org x, org y, org z}, double {L}, then vcode u64[V], first_child i32[N],
//        parent i32[N], corner f64[3N], edge f64[N], origins f64[3n], directions f64[3n], t_min f64[n], t_free f64[n],
//        t_end f64[n]
//   out: through u32[N], hits u32[N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "raycast_walk.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "evidence_host: the input ends early\n");
    exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const auto h = take<int64_t>(in, 7);
  const auto g = take<double>(in, 1);
  const int64_t V = h[1], N = h[2], n = h[3];
  const auto vcode = take<uint64_t>(in, (size_t)V);
  const auto first_child = take<int32_t>(in, (size_t)N), parent = take<int32_t>(in, (size_t)N);
  const auto corner = take<double>(in, (size_t)N * 3), edge = take<double>(in, (size_t)N);
  const auto org = take<double>(in, (size_t)n * 3), dir = take<double>(in, (size_t)n * 3);
  const auto t_min = take<double>(in, (size_t)n), t_free = take<double>(in, (size_t)n);
  const auto t_end = take<double>(in, (size_t)n);
  fclose(in);

  std::vector<uint32_t> through((size_t)N, 0u), hits((size_t)N, 0u);
  EvidenceTables T;
  T.t.mode = (int)h[0];
  T.t.L = g[0];
  T.t.org.x = (int32_t)h[4], T.t.org.y = (int32_t)h[5], T.t.org.z = (int32_t)h[6];
  T.t.vcode = vcode.data();
  T.t.V = V;
  T.t.first_child = first_child.data();
  T.t.corner = corner.data();
  T.t.edge = edge.data();
  T.parent = parent.data();
  T.max_steps = 4 * N + 64;
  T.through = through.data();
  T.hits = hits.data();

  for (int64_t i = 0; i < n; ++i)
    ray_evidence(T, &org[3 * i], &dir[3 * i], t_min[(size_t)i], t_free[(size_t)i], t_end[(size_t)i]);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  fwrite(through.data(), 4, (size_t)N, out);
  fwrite(hits.data(), 4, (size_t)N, out);
  return fclose(out) == 0 ? 0 : 2;
}
