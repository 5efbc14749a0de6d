// Stand-alone host program for tests/test_cpu_plane_cert.py: runs the certificate of octreelib_amd/csrc/plane_cert.h
// (the code k_ransac runs, compiled for the CPU) over the blocks of one file and writes its verdicts to another.
// Every block is a heap array of exactly its size, so a build with -fsanitize=address,undefined turns a read outside a
// block into an error.  No GPU, no HIP call.
//
//   plane_cert_host <in> <out>
//   in:  int64 {blocks}, then per block int64 {n}, double {t}, double xyz[3 n]
//   out: per block uint8 {no plane holds all n points, no plane holds n - 1 of them}
// The nine raw sums are taken relative to the block's first point, one point after the other (the kernel sums them
// as a tree over the wavefront; the header's rounding allowance covers any order).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plane_cert.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "plane_cert_host: the input ends early\n");
    exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const int64_t blocks = take<int64_t>(in, 1)[0];
  std::vector<uint8_t> verdict;
  verdict.reserve((size_t)blocks * 2);
  for (int64_t b = 0; b < blocks; ++b) {
    const int64_t n = take<int64_t>(in, 1)[0];
    const double t = take<double>(in, 1)[0];
    if (n < 1 || n > 64) return 2;
    const std::vector<double> p = take<double>(in, (size_t)n * 3);
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
      const double x = p[3 * i] - p[0], y = p[3 * i + 1] - p[1], z = p[3 * i + 2] - p[2];
      s[0] += x; s[1] += y; s[2] += z;
      s[3] += x * x; s[4] += x * y; s[5] += x * z;
      s[6] += y * y; s[7] += y * z; s[8] += z * z;
    }
    const plane_cert::Scatter sc = plane_cert::scatter_from_sums((int)n, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]);
    bool others = true;
    for (int64_t j = 0; j < n; ++j)
      others = plane_cert::no_plane_holds_others(sc, (int)n, p[3 * j] - p[0], p[3 * j + 1] - p[1], p[3 * j + 2] - p[2], t) &&
               others;
    verdict.push_back(plane_cert::no_plane_holds_all(sc, (int)n, t) ? 1 : 0);
    verdict.push_back(others ? 1 : 0);
  }
  fclose(in);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  fwrite(verdict.data(), 1, verdict.size(), out);
  return fclose(out) == 0 ? 0 : 2;
}
