// Stand-alone host program for tests/test_cpu_point_term_host.py: runs the per-point term of the point-to-point
// registration system (octreelib_amd/csrc/reg_point_term.h, the code k_regp_partial runs, compiled for the CPU) over
// tuples read from one file and writes the rows to another.  Every array is a heap block of exactly its size, so a build
// with -fsanitize=address,undefined turns an index outside one into an error.  No GPU, no HIP call.
//
//   point_term_host <in> <out>
//   in:  int64 n, then n rows of 10 f64: p[3], m[3], c[3], delta (<= 0: no Huber weights)
//   out: n rows of 28 f64 - the term of tuple i alone, entered into zeroed sums and expanded -, then one row of 28: all
//        tuples entered into the same sums in file order, expanded once
// e = p - m and d2 = (ex ex + ey ey) + ez ez are formed here as the search forms them (one rounding per operation; the
// build passes -ffp-contract=off), delta2 = delta delta as the library's host side does.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reg_point_term.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int64_t n = 0;
  if (fread(&n, sizeof n, 1, in) != 1 || n < 0 || n > (1 << 20)) return 2;
  std::vector<double> rows((size_t)n * 10);
  if (n && fread(rows.data(), sizeof(double), rows.size(), in) != rows.size()) {
    fprintf(stderr, "point_term_host: the input ends early\n");
    return 2;
  }
  fclose(in);
  std::vector<double> out((size_t)(n + 1) * 28);
  std::vector<double> all(RP_SUMS, 0.0);
  for (int64_t i = 0; i < n; ++i) {
    const double* t = rows.data() + (size_t)i * 10;
    const double p[3] = {t[0], t[1], t[2]}, c[3] = {t[6], t[7], t[8]};
    const double e[3] = {p[0] - t[3], p[1] - t[4], p[2] - t[5]};
    const double d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    const double delta = t[9] > 0.0 ? t[9] : 0.0;
    std::vector<double> one(RP_SUMS, 0.0);
    reg_point_term(p, c, e, d2, delta, delta * delta, one.data());
    reg_point_expand(one.data(), out.data() + (size_t)i * 28);
    reg_point_term(p, c, e, d2, delta, delta * delta, all.data());
  }
  reg_point_expand(all.data(), out.data() + (size_t)n * 28);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(out.data(), sizeof(double), out.size(), o);
  fclose(o);
  return 0;
}
