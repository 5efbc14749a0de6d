// Stand-alone host program for tests/test_cpu_ingest_transform_host.py: runs the per-thread body of k_ingest_xf
// (octreelib_amd/csrc/ingest_xf.h: ingest_xf_thread, the code the kernel runs, compiled for the CPU) for every
// "thread" of a launch over heap blocks that end exactly behind row n, so that a build with
// -fsanitize=address,undefined turns a read or write outside the cloud, the indices, the table or the store into an
// error.  No GPU, no HIP call.
//
//   ingest_xf_host <in> <out>
//   in:  int64 {n, f32, seg, M, dst_odd, src_off, in_place}, double table[12 M], uint16 segment[n] (seg != 0), then the
//        cloud: float[3 n] or double[3 n]
//        dst_odd:  the store starts 8 bytes behind a 16-byte boundary (a pose behind an odd number of rows)
//        src_off:  the cloud starts one element (8 / 4 bytes) behind a 16-byte boundary
//        in_place: f64 only - the cloud is copied into the store and moved there (src == dst)
//   out: double[3 n] the stored rows, then int64 rows folded
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ingest_xf.h"

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "ingest_xf_host: the input ends early\n");
    exit(2);
  }
  return v;
}

struct CountFold {
  int64_t rows = 0;
  void row(double, double, double) { ++rows; }
};

template <bool F32, bool SEG, bool SRC16, bool DST16>
static int64_t launch_as(const void* src, double* dst, const uint16_t* seg, const IxfMat* table, int M, int64_t n) {
  const int64_t per_wg = ixf_rows_per_wg<F32>();
  const int64_t blocks = (n + per_wg - 1) / per_wg;
  CountFold fold;
  for (int64_t b = 0; b < blocks; ++b)
    for (int t = 0; t < 256; ++t)
      ingest_xf_thread<F32, SEG, SRC16, DST16>(src, dst, seg, table[0], table, M, n, b * (256 * IXF_GROUPS) + t, fold);
  return fold.rows;
}

// the instance the library would launch for these two addresses
template <bool F32, bool SEG>
static int64_t launch(const void* src, double* dst, const uint16_t* seg, const IxfMat* table, int M, int64_t n) {
  const bool src16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0, dst16 = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  if (src16) return dst16 ? launch_as<F32, SEG, true, true>(src, dst, seg, table, M, n)
                          : launch_as<F32, SEG, true, false>(src, dst, seg, table, M, n);
  return dst16 ? launch_as<F32, SEG, false, true>(src, dst, seg, table, M, n)
               : launch_as<F32, SEG, false, false>(src, dst, seg, table, M, n);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const auto h = take<int64_t>(in, 7);
  const int64_t n = h[0];
  const bool f32 = h[1] != 0, seg = h[2] != 0, dst_odd = h[4] != 0, src_off = h[5] != 0, in_place = h[6] != 0;
  const int M = (int)h[3];
  if (n < 0 || M < 1 || (in_place && f32)) return 2;
  const auto tab = take<double>(in, (size_t)M * 12);
  const auto sidx = take<uint16_t>(in, seg ? (size_t)n : 0);
  const size_t esz = f32 ? 4 : 8, cloud_bytes = (size_t)n * 3 * esz;
  const auto cloud = take<char>(in, cloud_bytes);
  fclose(in);

  // heap blocks that end exactly behind the last element (malloc: 16-byte aligned)
  IxfMat* table = static_cast<IxfMat*>(malloc((size_t)M * sizeof(IxfMat)));
  memcpy(table, tab.data(), (size_t)M * sizeof(IxfMat));
  uint16_t* sdev = seg ? static_cast<uint16_t*>(malloc((size_t)n * 2 + (n == 0))) : nullptr;
  if (seg && n) memcpy(sdev, sidx.data(), (size_t)n * 2);
  const size_t s_pad = src_off ? esz : 0, d_pad = dst_odd ? 8 : 0;
  char* sbase = static_cast<char*>(malloc(cloud_bytes + s_pad + (cloud_bytes + s_pad == 0)));
  char* dbase = static_cast<char*>(malloc((size_t)n * 24 + d_pad + ((size_t)n * 24 + d_pad == 0)));
  if (n) memcpy(sbase + s_pad, cloud.data(), cloud_bytes);
  double* dst = reinterpret_cast<double*>(dbase + d_pad);
  const void* src = sbase + s_pad;
  if (in_place) {
    if (n) memcpy(dst, cloud.data(), cloud_bytes);
    src = dst;
  }
  int64_t rows;
  if (f32)
    rows = seg ? launch<true, true>(src, dst, sdev, table, M, n) : launch<true, false>(src, dst, sdev, table, M, n);
  else
    rows = seg ? launch<false, true>(src, dst, sdev, table, M, n) : launch<false, false>(src, dst, sdev, table, M, n);

  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  if (n) fwrite(dst, 8, (size_t)n * 3, out);
  fwrite(&rows, 8, 1, out);
  free(table);
  free(sdev);
  free(sbase);
  free(dbase);
  return fclose(out) == 0 ? 0 : 2;
}
