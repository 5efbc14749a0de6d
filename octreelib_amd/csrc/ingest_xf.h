// The per-thread body of k_ingest_xf (store.hip): the rows of a new pose read from the caller's cloud (f64 or f32),
// moved by their 3x4 and written into the forest's f64 store.  Host and device code: tests/host/ingest_xf_host.cpp
// runs the same body over heap buffers of exactly n rows under AddressSanitizer and UBSan.
//
// A row becomes ((m0 x + m1 y) + m2 z) + m3 per output coordinate - registration.py: transform_rows_np, every product
// and sum rounded (the library and the host program are built with -ffp-contract=off).
// A lane holds WHOLE rows, in groups that are a whole number of 16-byte units: two f64 rows = three double2, four f32
// rows = three float4 in and six double2 out.  Thread t of the launch owns the groups t, t + 256 within its workgroup's
// stretch (IXF_GROUPS of them: consecutive lanes read consecutive 48 bytes); the n mod rows-per-group rows behind the
// last whole group are the tail of the launch's first thread.  Everything a thread reads - its groups, its tail, its
// segment indices - is loaded before its first store: the f64 host form is uploaded into the store itself and moved in
// place (src == dst), and no thread reads a row of another.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

constexpr int IXF_GROUPS = 2;  // row groups per thread
template <bool F32>
constexpr int ixf_rows_per_group() { return F32 ? 4 : 2; }
template <bool F32>
constexpr int ixf_rows_per_wg() { return 256 * IXF_GROUPS * ixf_rows_per_group<F32>(); }  // 1024 (f64), 2048 (f32)

struct IxfMat {
  double m[12];  // rows (R_i0 R_i1 R_i2 t_i)
};

__host__ __device__ inline void ixf_apply(const double* m, double x, double y, double z, double* out) {
  out[0] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  out[1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  out[2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// an index beyond the table reads its last matrix (the Python layer has refused it; no read leaves the table)
__host__ __device__ inline int ixf_clamp(int s, int n_tab) { return s < n_tab ? s : n_tab - 1; }

// Do all rows of this group in all lanes of the wave share one matrix?  Every lane of the wave calls this, also a lane
// without a group (has == false: it agrees with anything).  Lanes hold ascending groups, so the first lane has a
// group whenever any lane has one.  *first is wave-uniform: the matrix is fetched once for the wave.  On the host a
// "wave" is one thread.
__host__ __device__ inline bool ixf_wave_agrees(bool has, bool same_in_thread, int s0, int* first) {
#if defined(__HIP_DEVICE_COMPILE__)
  *first = __builtin_amdgcn_readfirstlane(has ? s0 : 0);
  return __all(!has || (same_in_thread && s0 == *first)) != 0;
#else
  *first = s0;
  return has && same_in_thread;
#endif
}

// Fold: row(x, y, z) is called once for every row the thread stored, with the moved coordinates.
// SRC16 / DST16: the cloud / the new rows' place in the store start on a 16-byte boundary, so every group does - 16-byte
// accesses; otherwise element by element (8 or 4 bytes).  Compile-time, one kernel instance each: as run-time branches
// the compiler folds the two forms of a load into the narrower one.
template <bool F32, bool SEG, bool SRC16, bool DST16, class Fold>
__host__ __device__ inline void ingest_xf_thread(const void* src_v, double* dst, const uint16_t* seg,
                                                 const IxfMat& one, const IxfMat* table, int n_tab, int64_t n,
                                                 int64_t g0 /* the thread's first group */, Fold& fold) {
  using S = typename std::conditional<F32, float, double>::type;
  constexpr int RPG = ixf_rows_per_group<F32>(), VPG = 3 * RPG, TAIL = RPG - 1;
  const S* src = static_cast<const S*>(src_v);
  const int64_t n_groups = n / RPG;
  S v[IXF_GROUPS][VPG];
  int s[IXF_GROUPS][RPG];
  // ---- every load of the thread ---------------------------------------------------------------------------------
#pragma unroll
  for (int k = 0; k < IXF_GROUPS; ++k) {
    const int64_t g = g0 + k * 256;
#pragma unroll
    for (int j = 0; j < RPG; ++j) s[k][j] = 0;
    if (g < n_groups) {
      if constexpr (SRC16) {
        if constexpr (F32) {
          const float4* s4 = reinterpret_cast<const float4*>(src) + 3 * g;
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const float4 t = s4[u];
            v[k][4 * u] = t.x, v[k][4 * u + 1] = t.y, v[k][4 * u + 2] = t.z, v[k][4 * u + 3] = t.w;
          }
        } else {
          const double2* s2 = reinterpret_cast<const double2*>(src) + 3 * g;
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const double2 t = s2[u];
            v[k][2 * u] = t.x, v[k][2 * u + 1] = t.y;
          }
        }
      } else {
        const S* s1 = src + VPG * g;
#pragma unroll
        for (int u = 0; u < VPG; ++u) v[k][u] = s1[u];
      }
      if (SEG) {
#pragma unroll
        for (int j = 0; j < RPG; ++j) s[k][j] = ixf_clamp((int)seg[RPG * g + j], n_tab);
      }
    }
  }
  // the tail of the launch: the rows behind the last whole group
  const int64_t r_tail = n_groups * RPG;
  const int n_tail = g0 == 0 ? (int)(n - r_tail) : 0;
  S tv[TAIL][3];
  int ts[TAIL];
#pragma unroll
  for (int j = 0; j < TAIL; ++j) {
    ts[j] = 0;
    if (j < n_tail) {
      const S* s1 = src + 3 * (r_tail + j);
      tv[j][0] = s1[0], tv[j][1] = s1[1], tv[j][2] = s1[2];
      if (SEG) ts[j] = ixf_clamp((int)seg[r_tail + j], n_tab);
    }
  }
  // ---- move and store -------------------------------------------------------------------------------------------
  double m[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) m[c] = one.m[c];
  int cur = -1;  // (SEG: the table row m holds)
#pragma unroll
  for (int k = 0; k < IXF_GROUPS; ++k) {
    const int64_t g = g0 + k * 256;
    const bool has = g < n_groups;
    bool wave_one = false;
    if (SEG) {
      bool same = true;
#pragma unroll
      for (int j = 1; j < RPG; ++j) same = same && s[k][j] == s[k][0];
      int first;
      wave_one = ixf_wave_agrees(has, same, s[k][0], &first);
      if (wave_one && cur != first) {  // (one fetch for the wave: `first` is uniform)
#pragma unroll
        for (int c = 0; c < 12; ++c) m[c] = table[first].m[c];
        cur = first;
      }
    }
    if (!has) continue;
    double o[VPG];
#pragma unroll
    for (int j = 0; j < RPG; ++j) {
      if (SEG && !wave_one && s[k][j] != cur) {  // the per-lane gather
        cur = s[k][j];
#pragma unroll
        for (int c = 0; c < 12; ++c) m[c] = table[cur].m[c];
      }
      ixf_apply(m, (double)v[k][3 * j], (double)v[k][3 * j + 1], (double)v[k][3 * j + 2], &o[3 * j]);
      fold.row(o[3 * j], o[3 * j + 1], o[3 * j + 2]);
    }
    if constexpr (DST16) {
      double2* d2 = reinterpret_cast<double2*>(dst) + (VPG / 2) * g;
#pragma unroll
      for (int u = 0; u < VPG / 2; ++u) d2[u] = make_double2(o[2 * u], o[2 * u + 1]);
    } else {
      double* d1 = dst + VPG * g;
#pragma unroll
      for (int u = 0; u < VPG; ++u) d1[u] = o[u];
    }
  }
#pragma unroll
  for (int j = 0; j < TAIL; ++j) {
    if (j < n_tail) {
      if (SEG && ts[j] != cur) {
        cur = ts[j];
#pragma unroll
        for (int c = 0; c < 12; ++c) m[c] = table[cur].m[c];
      }
      double o[3];
      ixf_apply(m, (double)tv[j][0], (double)tv[j][1], (double)tv[j][2], o);
      fold.row(o[0], o[1], o[2]);
      double* d1 = dst + 3 * (r_tail + j);
      d1[0] = o[0], d1[1] = o[1], d1[2] = o[2];
    }
  }
}
