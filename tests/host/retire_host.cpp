// Stand-alone host program for tests/test_cpu_retire_host.py: applies the row map of octl_forest_remove_poses
// (octreelib_amd/csrc/store_retire.h, the code k_retire_poses runs, compiled for the CPU) to a store read from one file
// and writes the squeezed store to another.  Every array is a heap block of exactly its size, so a build with
// -fsanitize=address,undefined turns a row outside the old or the new store into an error.  No GPU, no HIP call.
//
//   retire_host <in> <out> <rows per tile>
//   in:  int64 {P, n_old}, end i64[P], shift i64[P + 1], xyz f64[3 n_old], alive u8[n_old]
//   out: int64 {n_new}, xyz f64[3 n_new], alive u8[n_new], new row of every old row i64[n_old] (-1: removed)
// The new store is filled tile by tile as the kernel's workgroups fill it: the poses of a tile's first and last row
// bracket the search for every double of the tile.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "store_retire.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "retire_host: the input ends early\n");
    exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const int64_t tile = atoll(argv[3]);
  const auto h = take<int64_t>(in, 2);
  const int P = (int)h[0];
  const int64_t n_old = h[1];
  const auto end = take<int64_t>(in, (size_t)P), shift = take<int64_t>(in, (size_t)P + 1);
  const auto xyz = take<double>(in, (size_t)n_old * 3);
  const auto alive = take<uint8_t>(in, (size_t)n_old);
  fclose(in);
  if (tile < 1 || P < 1 || end[(size_t)P - 1] != n_old) return 2;

  const RetireMap m{end.data(), shift.data(), P};
  const int64_t n_new = n_old - shift[(size_t)P];
  std::vector<double> out_xyz((size_t)n_new * 3);
  std::vector<uint8_t> out_alive((size_t)n_new);
  for (int64_t row0 = 0; row0 < n_new; row0 += tile) {
    const int64_t r_last = (row0 + tile < n_new ? row0 + tile : n_new) - 1;
    const int lo = retire_pose_of_new(m, 0, P - 1, row0);
    const int hi = retire_new_end(m, lo) > r_last ? lo : retire_pose_of_new(m, lo, P - 1, r_last);
    for (int64_t r = row0; r <= r_last; ++r) {
      const int p = lo == hi ? lo : retire_pose_of_new(m, lo, hi, r);
      out_alive[(size_t)r] = alive[(size_t)(r + shift[(size_t)p])];
      if (retire_old_row(m, r) != r + shift[(size_t)p]) return 3;   // (the bracketed search agrees with the full one)
    }
    for (int64_t d = 3 * row0; d < 3 * (r_last + 1); ++d)
      out_xyz[(size_t)d] = xyz[(size_t)retire_src_double(m, lo, hi, d)];
  }
  std::vector<int64_t> fwd((size_t)n_old);
  for (int64_t r = 0; r < n_old; ++r) {
    fwd[(size_t)r] = retire_new_row(m, r);
    if (fwd[(size_t)r] >= 0 && retire_old_row(m, fwd[(size_t)r]) != r) return 3;   // (the two maps are inverse)
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  fwrite(&n_new, 8, 1, out);
  fwrite(out_xyz.data(), 8, out_xyz.size(), out);
  fwrite(out_alive.data(), 1, out_alive.size(), out);
  fwrite(fwd.data(), 8, fwd.size(), out);
  return fclose(out) == 0 ? 0 : 2;
}
