// apply_mask: the stream compaction of the leaf-ordered arrays and of the block table by the RANSAC mask (or a
// filter's / carve's / the caller's mask), its asynchronous form and the C entries around the mask.
#include "forest.h"
#include "lookback.h"

namespace {

// ---- apply_mask: stream compaction of the leaf-ordered arrays and of the block table ----------------------
// kept points per 2048-point tile (the compaction's tile offsets) ...
__device__ __forceinline__ void mask_tile_count(const uint8_t* __restrict__ mask, int64_t n,
                                                uint32_t* __restrict__ tilecnt, uint32_t tile,
                                                uint8_t* __restrict__ alive_fill) {
  __shared__ uint32_t s_w[4];
  const int64_t i0 = (int64_t)tile * 2048 + (int64_t)threadIdx.x * 8;
  uint32_t c = 0;
  if (i0 + 8 <= n) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(mask + i0);  // (the mask buffer is 16-byte aligned)
    // bytes that are not zero
    const uint64_t nz = ((w & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | w;
    c = (uint32_t)__popcll(nz & 0x8080808080808080ull);
    // (alive flags that were never written - a cloud taken in place: position range = store range)
    if (alive_fill) *reinterpret_cast<uint64_t*>(alive_fill + i0) = 0x0101010101010101ull;
  } else {
    for (int64_t i = i0; i < n; ++i) {
      c += mask[i] ? 1u : 0u;
      if (alive_fill) alive_fill[i] = 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tilecnt[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// ... and per (leaf, pose) block: the block table is compacted block-wise, not re-derived from the points.
// ONE launch for both counts: workgroups [0, nt) take a tile of 2048 points each, the rest 256 blocks each.
__global__ __launch_bounds__(256) void k_blk_kept(const uint8_t* __restrict__ mask, int64_t n, uint32_t nt,
                                                  uint32_t* __restrict__ tilecnt,
                                                  const uint32_t* __restrict__ blk_start,
                                                  const int32_t* __restrict__ blk_size, int64_t nb,
                                                  uint32_t* __restrict__ kept, uint32_t* __restrict__ nonempty,
                                                  uint8_t* __restrict__ alive_fill) {
  if (blockIdx.x < nt) {
    mask_tile_count(mask, n, tilecnt, blockIdx.x, alive_fill);
    return;
  }
  const int64_t b = (int64_t)(blockIdx.x - nt) * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t st = b < nb ? blk_start[b] : 0u;
  const int sz = b < nb ? blk_size[b] : 0;
  uint32_t c = 0;
  if (sz <= 256)
    for (int i = 0; i < sz; ++i) c += mask[(size_t)st + i] ? 1u : 0u;
  // large blocks (unsplit voxels, big leaves of a bare octree): the whole wave, one block at a time
  unsigned long long big = __ballot(sz > 256);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const uint32_t s0 = (uint32_t)__shfl((int)st, src);
    const int z = __shfl(sz, src);
    uint32_t cc = 0;
    for (int i = lane; i < z; i += 64) cc += mask[(size_t)s0 + i] ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cc += __shfl_xor(cc, off);
    if (lane == src) c = cc;
  }
  if (b < nb) {
    kept[b] = c;
    nonempty[b] = c ? 1u : 0u;
  }
}


// tile-wise stable compaction (8 rows of 256 points per workgroup, ballot ranks); dropped points die in the store.
// offset_of(kept points of the tile) -> kept points in front of the tile: read from the scanned table
// (k_compact_tiles) or found by look-back (the tile workgroups of k_mask_scan, small clouds: no launch of its own).
template <typename OffsetOf>
__device__ __forceinline__ void compact_tile(
    uint32_t tile, const uint8_t* __restrict__ mask, int64_t n,
    const uint32_t* __restrict__ ord_idx, const double* __restrict__ xyz_ord,
    uint32_t* __restrict__ ord_idx2, double* __restrict__ xyz_ord2, uint8_t* __restrict__ alive,
    uint8_t* __restrict__ alive_fill, uint32_t* s_cnt /* [33] */, OffsetOf offset_of) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t base = (int64_t)tile * 2048;
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t rk[8];
  uint32_t keepbits = 0;
  // (every load of the tile is issued before the first dependent instruction: 8 rounds x (index + 3 coordinates)
  //  in flight per lane; loading them behind `if (kept)` round by round left the kernel at 4.9 TB/s)
  uint32_t iv[8];
  double px[8], py[8], pz[8];
  uint8_t mk[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    mk[r] = 0;
    iv[r] = 0;
    px[r] = py[r] = pz[r] = 0.0;
    if (i < n) {
      mk[r] = mask[i];
      iv[r] = ord_idx[i];
      px[r] = xyz_ord[3 * i];
      py[r] = xyz_ord[3 * i + 1];
      pz[r] = xyz_ord[3 * i + 2];
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    const bool k = i < n && mk[r] != 0;
    const unsigned long long bal = __ballot(k);
    rk[r] = (uint32_t)__popcll(bal & lt);
    keepbits |= (k ? 1u : 0u) << r;
    if (lane == 0) s_cnt[r * 4 + wave] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    uint32_t v = lane < 32 ? s_cnt[lane] : 0u, inc = v;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      const uint32_t t = __shfl_up(inc, off);
      if (lane >= off) inc += t;
    }
    if (lane < 32) s_cnt[lane] = inc - v;
    if (lane == 31) s_cnt[32] = inc;  // kept points of the tile
  }
  __syncthreads();
  const uint32_t toff = offset_of(s_cnt[32]);
  // (alive flags that were never written: position range = store range, every flag of the tile is written here)
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    if (i >= n) continue;
    if ((keepbits >> r) & 1u) {
      const int64_t d = (int64_t)toff + s_cnt[r * 4 + wave] + rk[r];
      ord_idx2[d] = iv[r];
      xyz_ord2[3 * d] = px[r];
      xyz_ord2[3 * d + 1] = py[r];
      xyz_ord2[3 * d + 2] = pz[r];
      if (alive_fill) alive_fill[iv[r]] = 1;
    } else {
      alive[iv[r]] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void k_compact_tiles(
    const uint8_t* __restrict__ mask, const uint32_t* __restrict__ tile_off, int64_t n,
    const uint32_t* __restrict__ ord_idx, const double* __restrict__ xyz_ord,
    uint32_t* __restrict__ ord_idx2, double* __restrict__ xyz_ord2, uint8_t* __restrict__ alive) {
  __shared__ uint32_t s_cnt[33];  // [row][wave] -> exclusive offsets | total
  compact_tile(blockIdx.x, mask, n, ord_idx, xyz_ord, ord_idx2, xyz_ord2, alive, nullptr, s_cnt,
               [&](uint32_t) { return tile_off[blockIdx.x]; });
}


// apply_mask's counts, prefix sums and block-table compaction in ONE launch (round 5; before: k_blk_kept, a scan over
// [tile counts | kept per block | block non-empty], k_blk_compact).  Workgroups [0, nt) take a tile of 2048 positions:
// kept points of the tile, chained by decoupled look-back into the tile's offset, and the tile's compaction.
// Workgroups [nt, nt + nbw) take 256 blocks each: kept points and "non-empty" per block, two look-back chains over
// the block workgroups (kept points in front = the block's new start, non-empty blocks in front = its new id), and
// the surviving blocks are written straight into the compacted table.  Chains never cross: each has its own status
// words, and tiles are taken in blockIdx order inside every chain.  totals[0] / totals[1] (pinned host memory):
// kept points, surviving blocks.  fill_alive: the store's alive flags have never been written (a cloud taken in
// place): the tile workgroups write 1s over their range - position range = store range while every point is alive.
__global__ __launch_bounds__(256) void k_mask_scan(
    const uint8_t* __restrict__ mask, int64_t n, uint32_t nt,
    const uint32_t* __restrict__ ord_idx, const double* __restrict__ xyz_ord,
    uint32_t* __restrict__ ord_idx2, double* __restrict__ xyz_ord2, uint8_t* __restrict__ alive,
    const uint32_t* __restrict__ blk_start, const int32_t* __restrict__ blk_size, int64_t nb,
    const int32_t* __restrict__ blk_node, const int32_t* __restrict__ blk_slot, int32_t* __restrict__ blk_node2,
    int32_t* __restrict__ blk_slot2, uint32_t* __restrict__ blk_start2, int32_t* __restrict__ blk_size2,
    uint64_t* __restrict__ st_tiles, uint64_t* __restrict__ st_kept, uint64_t* __restrict__ st_ids, uint32_t epoch,
    uint32_t* __restrict__ mirror, uint32_t seq, uint8_t* __restrict__ alive_fill) {
  __shared__ uint32_t s_w[2][4];
  __shared__ uint32_t s_excl;
  __shared__ uint32_t s_cnt[33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x < nt) {
    // a tile of 2048 positions: its loads are in flight while the look-back finds the kept points in front of it,
    // then it compacts itself (round 6: was a count here and k_compact_tiles behind - one launch more)
    const uint32_t tile = blockIdx.x;
    compact_tile(tile, mask, n, ord_idx, xyz_ord, ord_idx2, xyz_ord2, alive, alive_fill, s_cnt,
                 [&](uint32_t total) {
                   const uint32_t excl = lookback_exclusive(st_tiles, epoch, tile, total, &s_excl);
                   if (threadIdx.x == 0 && tile == nt - 1) {
                     mirror[MIRROR_MASK_TOTALS] = excl + total;
                     mirror_publish(mirror, MIRROR_FLAG_MASK0, seq);
                   }
                   return excl;
                 });
    return;
  }
  const uint32_t bw = blockIdx.x - nt;
  const int64_t b = (int64_t)bw * 256 + threadIdx.x;
  const uint32_t st = b < nb ? blk_start[b] : 0u;
  const int sz = b < nb ? blk_size[b] : 0;
  uint32_t c = 0;
  if (sz <= 256)
    for (int i = 0; i < sz; ++i) c += mask[(size_t)st + i] ? 1u : 0u;
  // large blocks (unsplit voxels, big leaves of a bare octree): the whole wave, one block at a time
  unsigned long long big = __ballot(sz > 256);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    const uint32_t s0 = (uint32_t)__shfl((int)st, src);
    const int z = __shfl(sz, src);
    uint32_t cc = 0;
    for (int i = lane; i < z; i += 64) cc += mask[(size_t)s0 + i] ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cc += __shfl_xor(cc, off);
    if (lane == src) c = cc;
  }
  // exclusive prefixes inside the workgroup: kept points, non-empty blocks
  const uint32_t ne = c ? 1u : 0u;
  uint32_t ic = c, ie = ne;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t tc = __shfl_up(ic, off), te = __shfl_up(ie, off);
    if (lane >= off) {
      ic += tc;
      ie += te;
    }
  }
  if (lane == 63) {
    s_w[0][wave] = ic;
    s_w[1][wave] = ie;
  }
  __syncthreads();
  uint32_t pc = ic - c, pe = ie - ne, tot_c = 0, tot_e = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) {
      pc += s_w[0][w];
      pe += s_w[1][w];
    }
    tot_c += s_w[0][w];
    tot_e += s_w[1][w];
  }
  __syncthreads();   // (s_excl is used by both chains)
  const uint32_t ex_c = lookback_exclusive(st_kept, epoch, bw, tot_c, &s_excl);
  __syncthreads();
  const uint32_t ex_e = lookback_exclusive(st_ids, epoch, bw, tot_e, &s_excl);
  if (threadIdx.x == 0 && bw == gridDim.x - nt - 1) {
    mirror[MIRROR_MASK_TOTALS + 1] = ex_e + tot_e;
    mirror_publish(mirror, MIRROR_FLAG_MASK1, seq);
  }
  if (b < nb && c) {
    const uint32_t id = ex_e + pe;
    blk_node2[id] = blk_node[b];
    blk_slot2[id] = blk_slot[b];
    blk_start2[id] = ex_c + pc;
    blk_size2[id] = (int32_t)c;
  }
}

// The three prefix sums of apply_mask come out of ONE scan over [tile counts | kept per block | block
// non-empty]: the second and third segment carry the totals of the segments in front of them, which are
// read from their first entries.
__global__ __launch_bounds__(256) void k_blk_compact(
    const uint32_t* __restrict__ raw, const uint32_t* __restrict__ scanned, const uint32_t* __restrict__ grand_total,
    int64_t nt, int64_t nb, const int32_t* __restrict__ blk_node,
    const int32_t* __restrict__ blk_slot, int32_t* __restrict__ blk_node2, int32_t* __restrict__ blk_slot2,
    uint32_t* __restrict__ blk_start2, int32_t* __restrict__ blk_size2, uint32_t* __restrict__ mirror,
    uint32_t seq) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t base_kept = scanned[nt], base_id = scanned[nt + nb];
  if (b == 0) {
    mirror[MIRROR_MASK_TOTALS] = base_id - base_kept;          // kept points
    mirror[MIRROR_MASK_TOTALS + 1] = *grand_total - base_id;   // non-empty blocks
    mirror_publish(mirror, MIRROR_FLAG_MASK0, seq);
    mirror_publish(mirror, MIRROR_FLAG_MASK1, seq);
  }
  if (b >= nb) return;
  const uint32_t c = raw[nt + b];
  if (!c) return;
  const uint32_t id = scanned[nt + nb + b] - base_id;
  blk_node2[id] = blk_node[b];
  blk_slot2[id] = blk_slot[b];
  blk_start2[id] = scanned[nt + b] - base_kept;
  blk_size2[id] = (int32_t)c;
}

// OctreeNode.filter for count predicates (octree.py:102-112): a leaf of a selected pose whose point
// count lies outside [lo, hi] is emptied - one wavefront per block clears its mask bytes
__global__ __launch_bounds__(256) void k_filter_blocks(const uint32_t* __restrict__ blk_start,
                                                       const int32_t* __restrict__ blk_size,
                                                       const int32_t* __restrict__ blk_slot, int64_t nb,
                                                       const uint8_t* __restrict__ slot_sel, int64_t lo,
                                                       int64_t hi, uint8_t* __restrict__ mask) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  const int64_t n = blk_size[b];
  if (!slot_sel[blk_slot[b]] || (n >= lo && n <= hi)) return;
  const int64_t s0 = blk_start[b];
  for (int64_t i = threadIdx.x & 63; i < n; i += 64) mask[s0 + i] = 0;
}

// octl_forest_carve: a (leaf, pose) block of a selected pose (slot_sel nullptr: every pose) whose leaf at least
// min_through rays passed through and at most max_hits rays ended in (the counters of octl_forest_ray_evidence, one
// pair per node) is emptied - query.py: carve_keep_np is the rule.  One wavefront per block clears its mask bytes.
__global__ __launch_bounds__(256) void k_carve_blocks(const uint32_t* __restrict__ blk_start,
                                                      const int32_t* __restrict__ blk_size,
                                                      const int32_t* __restrict__ blk_slot,
                                                      const int32_t* __restrict__ blk_node, int64_t nb,
                                                      const uint8_t* __restrict__ slot_sel,
                                                      const uint32_t* __restrict__ through,
                                                      const uint32_t* __restrict__ hits, int64_t min_through,
                                                      int64_t max_hits, uint8_t* __restrict__ mask) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;
  if (slot_sel && !slot_sel[blk_slot[b]]) return;
  const int32_t node = blk_node[b];
  if (!((int64_t)through[node] >= min_through && (int64_t)hits[node] <= max_hits)) return;
  const int64_t n = blk_size[b], s0 = blk_start[b];
  for (int64_t i = threadIdx.x & 63; i < n; i += 64) mask[s0 + i] = 0;
}

// octl_forest_remove_poses (store_retire.h): a (leaf, pose) block of a pose that leaves is emptied and its size
// counted; fill: no mask is pending, so the bytes of every other block become 1 here - the blocks cover the ordered
// points exactly - instead of in a fill launch.  One wavefront per block, over a grid that stops growing at 2048
// workgroups: the sizes are summed per workgroup and added to *removed with ONE atomic each (same-address atomics
// serialise; one per block of a removed pose would be tens of thousands).
__global__ __launch_bounds__(256) void k_retire_mask(const uint32_t* __restrict__ blk_start,
                                                     const int32_t* __restrict__ blk_size,
                                                     const int32_t* __restrict__ blk_slot, int64_t nb,
                                                     const uint8_t* __restrict__ slot_sel, int fill,
                                                     uint8_t* __restrict__ mask,
                                                     unsigned long long* __restrict__ removed) {
  __shared__ unsigned long long s_gone[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned long long gone = 0;   // (wave-uniform)
  for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < nb; b += (int64_t)gridDim.x * 4) {
    const bool leaves = slot_sel[blk_slot[b]] != 0;
    if (!leaves && !fill) continue;
    const int64_t n = blk_size[b], s0 = blk_start[b];
    const uint8_t v = leaves ? 0 : 1;
    for (int64_t i = lane; i < n; i += 64) mask[s0 + i] = v;
    if (leaves) gone += (unsigned long long)n;
  }
  if (lane == 0) s_gone[wave] = gone;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long all = s_gone[0] + s_gone[1] + s_gone[2] + s_gone[3];
    if (all) atomicAdd(removed, all);
  }
}

// The block table describes the leaf-ordered arrays exactly (every producer leaves it that way), so both
// are compacted together: points tile-wise, blocks block-wise.  One synchronisation (kept points, blocks).
// (async: return behind the last launch - forest_settle books the counts when somebody looks at the forest again)
int apply_device_mask(octl_forest* f, int64_t* n_alive_out, bool async = false) {
  octl_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  // (the counts travel through two words of the context's mirror: one compaction in flight per context)
  if (ctx->pending_mask_forest && ctx->pending_mask_forest != f) OCTL_TRY(forest_settle(ctx->pending_mask_forest));
  OCTL_TRY(forest_settle(f));
  const int64_t n = f->n_ord, nb = f->n_blocks;
  f->mask_valid = false;
  f->fast_order_valid = false;  // block ids change
  forest_contents_changed(f);  // (the points that are about to leave)
  if (n > 0 && nb > 0) {
    KTimer t(ctx, "apply_mask");
    uint32_t* small = ctx->small.as<uint32_t>();
    const int64_t nt = ceil_div(n, 2048);
    // scratch: in [tile counts nt | kept nb | non-empty nb], out (scanned) the same layout
    const int64_t n_all = nt + 2 * nb;
    const size_t o_out = (((size_t)n_all + 8) * 4 + 15) & ~(size_t)15;
    OCTL_TRY(devbuf_reserve(ctx, f->flags, 2 * o_out));
    uint32_t* raw = f->flags.as<uint32_t>();
    uint32_t* scanned = reinterpret_cast<uint32_t*>(static_cast<char*>(f->flags.p) + o_out);
    const uint8_t* mask = f->mask.as<uint8_t>();
    // the fused form chains its workgroups by look-back: beyond ~1000 of them the chain costs more than the
    // separate scan (10 M points: 65 us against 35)
    const bool fused = !ctx->opt.no_fused_tables && nt + 2 * ceil_div(nb, 256) <= 1024;
    const uint32_t wait_seq = octl_wait_next_seq(ctx);
    // (alive flags that were never written - a cloud taken in place - are filled by the tile workgroups of the
    //  first kernel: by position in k_blk_kept - k_compact_tiles, a later launch, then clears the dropped points' -
    //  and by store index, each flag once, where k_mask_scan compacts in the same launch)
    uint8_t* fill = nullptr;
    if (f->alive_stale && f->n_ord == f->n_store) {
      fill = f->alive.as<uint8_t>();
      f->alive_stale = false;
    } else {
      OCTL_TRY(alive_ensure(f));
    }
    if (!fused) {
      OCTL_LAUNCH(k_blk_kept, dim3((unsigned)nt + grid_for(nb)), dim3(256), 0, st, mask, n, (uint32_t)nt, raw,
                         (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(), nb,
                         raw + nt, raw + nt + nb, fill);
      HIP_TRY(ctx, hipGetLastError());
      OCTL_TRY(octl_exclusive_scan_u32(ctx, raw, scanned, n_all, small + SM_MASK_TOTAL));
    }
    OCTL_TRY(devbuf_reserve(ctx, f->ord_idx2, (size_t)n * 4));
    OCTL_TRY(devbuf_reserve(ctx, f->xyz_ord2, (size_t)n * 24));
    // (block buffers keep the capacity convention of forest_make_blocks: one block per point)
    OCTL_TRY(devbuf_reserve(ctx, f->blk_node2, (size_t)n * 4));
    OCTL_TRY(devbuf_reserve(ctx, f->blk_slot2, (size_t)n * 4));
    OCTL_TRY(devbuf_reserve(ctx, f->blk_start2, (size_t)n * 4));
    OCTL_TRY(devbuf_reserve(ctx, f->blk_size2, (size_t)n * 4));
    if (fused) {
      // counts + the three prefix sums + the block table's compaction: one launch (k_mask_scan)
      const int64_t nbw = ceil_div(nb, 256);
      uint64_t* status = nullptr;
      uint32_t epoch = 0;
      OCTL_TRY(octl_scan_status_acquire(ctx, nt + 2 * nbw, &status, &epoch));
      OCTL_LAUNCH(k_mask_scan, dim3((unsigned)(nt + nbw)), dim3(256), 0, st, mask, n, (uint32_t)nt,
                         (const uint32_t*)f->ord_idx.as<uint32_t>(), (const double*)f->xyz_ord.as<double>(),
                         f->ord_idx2.as<uint32_t>(), f->xyz_ord2.as<double>(), f->alive.as<uint8_t>(),
                         (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(), nb,
                         (const int32_t*)f->blk_node.as<int32_t>(), (const int32_t*)f->blk_slot.as<int32_t>(),
                         f->blk_node2.as<int32_t>(), f->blk_slot2.as<int32_t>(), f->blk_start2.as<uint32_t>(),
                         f->blk_size2.as<int32_t>(), status, status + nt, status + nt + nbw, epoch,
                         static_cast<uint32_t*>(ctx->small_host), wait_seq, fill);
      HIP_TRY(ctx, hipGetLastError());
    }
    if (!fused) {
      OCTL_LAUNCH(k_compact_tiles, dim3((unsigned)nt), dim3(256), 0, st, mask, (const uint32_t*)scanned, n,
                         (const uint32_t*)f->ord_idx.as<uint32_t>(), (const double*)f->xyz_ord.as<double>(),
                         f->ord_idx2.as<uint32_t>(), f->xyz_ord2.as<double>(), f->alive.as<uint8_t>());
      HIP_TRY(ctx, hipGetLastError());
      OCTL_LAUNCH(k_blk_compact, dim3(grid_for(nb)), dim3(256), 0, st, (const uint32_t*)raw,
                         (const uint32_t*)scanned, (const uint32_t*)(small + SM_MASK_TOTAL), nt, nb,
                         (const int32_t*)f->blk_node.as<int32_t>(), (const int32_t*)f->blk_slot.as<int32_t>(),
                         f->blk_node2.as<int32_t>(), f->blk_slot2.as<int32_t>(), f->blk_start2.as<uint32_t>(),
                         f->blk_size2.as<int32_t>(), static_cast<uint32_t*>(ctx->small_host), wait_seq);
      HIP_TRY(ctx, hipGetLastError());
    }
    // (the two totals and their flags are written into the pinned mirror by the kernels themselves: the host polls
    //  for them - the compaction of the points may still be running when this returns, everything behind it is
    //  ordered by the stream)
    std::swap(f->ord_idx, f->ord_idx2);
    std::swap(f->xyz_ord, f->xyz_ord2);
    std::swap(f->blk_node, f->blk_node2);
    std::swap(f->blk_slot, f->blk_slot2);
    std::swap(f->blk_start, f->blk_start2);
    std::swap(f->blk_size, f->blk_size2);
    f->totals_pending = true;
    f->totals_seq = wait_seq;
    f->totals_n_before = n;
    ctx->pending_mask_forest = f;
    if (!async) OCTL_TRY(forest_settle(f));
  }
  if (n_alive_out) *n_alive_out = f->n_ord;
  return OCTL_OK;
}

// both forms of octl_forest_carve: the refusals, the counters (uploaded into f->q_stage by the host form), the blocks
// cleared in the mask - a pending RANSAC mask stays in it, as with octl_forest_filter_count - and ONE compaction
int forest_carve(octl_forest* f, const uint32_t* through, const uint32_t* hits, bool on_device, int64_t n_nodes,
                 const uint8_t* slot_sel, int32_t n_sel, int64_t min_through, int64_t max_hits, int64_t* n_alive) {
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "carve before build");
  const int64_t N = f->nodes[f->cur].n;
  if (n_nodes != N)
    return octl_set_error(ctx, OCTL_E_INVALID,
                          "carve: counters for %lld nodes, the scheme has %lld (evidence belongs to the scheme it "
                          "was taken on)",
                          (long long)n_nodes, (long long)N);
  if (N > 0 && (!through || !hits)) return octl_set_error(ctx, OCTL_E_INVALID, "bad carve arguments");
  if (min_through < 1)
    return octl_set_error(ctx, OCTL_E_INVALID, "carve: min_through = %lld is below 1", (long long)min_through);
  if (max_hits < 0)
    return octl_set_error(ctx, OCTL_E_INVALID, "carve: max_hits = %lld is negative", (long long)max_hits);
  std::vector<uint8_t> sel;
  OCTL_TRY(forest_selection(f, slot_sel, n_sel, &sel));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (f->n_blocks > 0) {
    // (every buffer first: a failed allocation leaves the mask as it was)
    if (!on_device) OCTL_TRY(devbuf_reserve(ctx, f->q_stage, (size_t)N * 8));
    if (!sel.empty()) OCTL_TRY(devbuf_reserve(ctx, f->scheme_dev, sel.size()));
    OCTL_TRY(ensure_mask(f));
    if (!on_device) {
      uint32_t* c_d = f->q_stage.as<uint32_t>();
      HIP_TRY(ctx, hipMemcpyAsync(c_d, through, (size_t)N * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(c_d + N, hits, (size_t)N * 4, hipMemcpyHostToDevice, st));
      through = c_d;
      hits = c_d + N;
    } else {
      OCTL_TRY(ctx_wait_uploads(ctx, through, (size_t)N * 4));
      OCTL_TRY(ctx_wait_uploads(ctx, hits, (size_t)N * 4));
    }
    if (!sel.empty())
      HIP_TRY(ctx, hipMemcpyAsync(f->scheme_dev.p, sel.data(), sel.size(), hipMemcpyHostToDevice, st));
    if (!on_device || !sel.empty()) HIP_TRY(ctx, hipStreamSynchronize(st));  // (pageable sources)
    KTimer t(ctx, "carve");
    OCTL_LAUNCH(k_carve_blocks, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st,
                (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                (const int32_t*)f->blk_slot.as<int32_t>(), (const int32_t*)f->blk_node.as<int32_t>(), f->n_blocks,
                sel.empty() ? (const uint8_t*)nullptr : (const uint8_t*)f->scheme_dev.as<uint8_t>(), through, hits,
                min_through, max_hits, f->mask.as<uint8_t>());
    HIP_TRY(ctx, hipGetLastError());
  } else {
    OCTL_TRY(ensure_mask(f));
  }
  return apply_device_mask(f, n_alive);
}

}  // namespace

// (the sizes apply_device_mask asks for, in its order: what is reserved here it does not grow)
int mask_retire_reserve(octl_forest* f) {
  octl_ctx* ctx = f->ctx;
  const int64_t n = f->n_ord, nb = f->n_blocks;
  OCTL_TRY(devbuf_reserve(ctx, f->mask, (size_t)std::max<int64_t>(n, 1), f->mask_valid ? 1 : 0));
  if (n <= 0 || nb <= 0) return OCTL_OK;
  const int64_t nt = ceil_div(n, 2048), n_all = nt + 2 * nb;
  const size_t o_out = (((size_t)n_all + 8) * 4 + 15) & ~(size_t)15;
  OCTL_TRY(devbuf_reserve(ctx, f->flags, 2 * o_out));
  if (!ctx->opt.no_fused_tables && nt + 2 * ceil_div(nb, 256) <= 1024)
    OCTL_TRY(octl_scan_status_reserve(ctx, nt + 2 * ceil_div(nb, 256)));
  else
    OCTL_TRY(octl_exclusive_scan_reserve(ctx, n_all));
  OCTL_TRY(devbuf_reserve(ctx, f->ord_idx2, (size_t)n * 4));
  OCTL_TRY(devbuf_reserve(ctx, f->xyz_ord2, (size_t)n * 24));
  OCTL_TRY(devbuf_reserve(ctx, f->blk_node2, (size_t)n * 4));
  OCTL_TRY(devbuf_reserve(ctx, f->blk_slot2, (size_t)n * 4));
  OCTL_TRY(devbuf_reserve(ctx, f->blk_start2, (size_t)n * 4));
  OCTL_TRY(devbuf_reserve(ctx, f->blk_size2, (size_t)n * 4));
  return OCTL_OK;
}

int mask_retire_slots(octl_forest* f, const uint8_t* sel_dev, unsigned long long* removed_dev) {
  octl_ctx* ctx = f->ctx;
  if (f->n_ord > 0 && f->n_blocks > 0) {
    KTimer t(ctx, "remove_poses");
    OCTL_LAUNCH(k_retire_mask, dim3((unsigned)std::min<int64_t>(ceil_div(f->n_blocks, 4), 2048)), dim3(256), 0, ctx->stream,
                (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                (const int32_t*)f->blk_slot.as<int32_t>(), f->n_blocks, sel_dev, f->mask_valid ? 0 : 1,
                f->mask.as<uint8_t>(), removed_dev);
    HIP_TRY(ctx, hipGetLastError());
    f->mask_valid = true;
  }
  return apply_device_mask(f, nullptr);
}

int mask_apply(octl_forest* f, int64_t* n_alive) { return apply_device_mask(f, n_alive); }

int forest_settle(octl_forest* f) {
  if (!f->totals_pending) return OCTL_OK;
  octl_ctx* ctx = f->ctx;
  f->totals_pending = false;
  if (ctx->pending_mask_forest == f) ctx->pending_mask_forest = nullptr;
  const int flags[2] = {MIRROR_FLAG_MASK0, MIRROR_FLAG_MASK1};
  const int64_t n = f->totals_n_before;
  OCTL_TRY(octl_wait_mirror_flags(ctx, flags, 2, f->totals_seq, 500 + n / 2000));
  uint32_t res[2];
  std::memcpy(res, static_cast<uint32_t*>(ctx->small_host) + MIRROR_MASK_TOTALS, 8);
  f->n_alive -= (n - (int64_t)res[0]);
  f->n_ord = res[0];
  f->n_blocks = res[1];
  return OCTL_OK;
}

void forest_forget_pending(octl_forest* f) {
  if (!f->totals_pending) return;
  f->totals_pending = false;
  if (f->ctx->pending_mask_forest == f) f->ctx->pending_mask_forest = nullptr;
}

int ensure_mask(octl_forest* f) {
  octl_ctx* ctx = f->ctx;
  if (f->mask_valid) return OCTL_OK;
  OCTL_TRY(devbuf_reserve(ctx, f->mask, (size_t)std::max<int64_t>(f->n_ord, 1)));
  if (f->n_ord > 0)
    HIP_TRY(ctx, hipMemsetAsync(f->mask.p, 1, (size_t)f->n_ord, ctx->stream));
  f->mask_valid = true;
  return OCTL_OK;
}

extern "C" {

int octl_forest_get_mask(octl_forest* f, int64_t cap, uint8_t* mask, int64_t* n_out) {
  if (!f || !n_out) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "no scheme has been built");
  *n_out = f->n_ord;
  const int64_t n = std::min<int64_t>(cap, f->n_ord);
  if (n <= 0 || !mask) return OCTL_OK;
  OCTL_TRY(ensure_mask(f));
  HIP_TRY(ctx, hipMemcpyAsync(mask, f->mask.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return OCTL_OK;
}

int octl_forest_apply_mask(octl_forest* f, int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  if (!f->built) return octl_set_error(f->ctx, OCTL_E_STATE, "apply_mask before build");
  AheadAllow allow(f->ctx);  // (see octl_forest_apply_mask_async)
  OCTL_TRY(ensure_mask(f));
  return apply_device_mask(f, n_alive);
}

int octl_forest_apply_mask_async(octl_forest* f) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  if (!f->built) return octl_set_error(f->ctx, OCTL_E_STATE, "apply_mask before build");
  // The compaction reads the mask, the leaf-ordered arrays and the block table, writes their second set, the alive
  // flags and f->flags, chains its workgroups over the status words of the context's stream and keeps its one scalar
  // (SM_MASK_TOTAL) outside the words a build's front writes: the partition front of the context's next build may run
  // on the ahead stream while it is in flight - that build takes no alive flags (every point of a cloud
  // taken in place is alive), so the fill of f->alive in here is not its concern either.
  AheadAllow allow(f->ctx);
  OCTL_TRY(ensure_mask(f));
  return apply_device_mask(f, nullptr, true);
}

int octl_forest_settle(octl_forest* f, int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  if (n_alive) *n_alive = f->n_ord;
  return OCTL_OK;
}

int octl_forest_filter_count(octl_forest* f, const uint8_t* slot_sel, int32_t n_sel, int64_t lo,
                             int64_t hi, int64_t* n_alive) {
  if (!f || !slot_sel) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "filter before build");
  const int n_poses = (int)f->pose_off.size() - 1;
  if (n_sel != n_poses) return octl_set_error(ctx, OCTL_E_INVALID, "slot selection has %d entries for %d poses", n_sel, n_poses);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OCTL_TRY(ensure_mask(f));
  if (f->n_blocks > 0) {
    OCTL_TRY(devbuf_reserve(ctx, f->scheme_dev, (size_t)std::max(n_poses, 1)));
    HIP_TRY(ctx, hipMemcpyAsync(f->scheme_dev.p, slot_sel, (size_t)n_poses, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (a pageable source)
    KTimer t(ctx, "filter");
    OCTL_LAUNCH(k_filter_blocks, dim3((unsigned)ceil_div(f->n_blocks, 4)), dim3(256), 0, st,
                       (const uint32_t*)f->blk_start.as<uint32_t>(), (const int32_t*)f->blk_size.as<int32_t>(),
                       (const int32_t*)f->blk_slot.as<int32_t>(), f->n_blocks,
                       (const uint8_t*)f->scheme_dev.as<uint8_t>(), lo, hi, f->mask.as<uint8_t>());
    HIP_TRY(ctx, hipGetLastError());
  }
  return apply_device_mask(f, n_alive);
}

int octl_forest_carve(octl_forest* f, const uint32_t* through, const uint32_t* hits, int64_t n_nodes,
                      const uint8_t* slot_sel, int32_t n_sel, int64_t min_through, int64_t max_hits,
                      int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  return forest_carve(f, through, hits, false, n_nodes, slot_sel, n_sel, min_through, max_hits, n_alive);
}

int octl_forest_carve_device(octl_forest* f, const uint32_t* through_dev, const uint32_t* hits_dev, int64_t n_nodes,
                             const uint8_t* slot_sel, int32_t n_sel, int64_t min_through, int64_t max_hits,
                             int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  return forest_carve(f, through_dev, hits_dev, true, n_nodes, slot_sel, n_sel, min_through, max_hits, n_alive);
}

int octl_forest_apply_host_mask(octl_forest* f, const uint8_t* mask, int64_t n, int64_t* n_alive) {
  if (!f) return OCTL_E_INVALID;
  OCTL_TRY(forest_settle(f));
  octl_ctx* ctx = f->ctx;
  if (!f->built) return octl_set_error(ctx, OCTL_E_STATE, "apply_mask before build");
  if (n != f->n_ord || (n > 0 && !mask))
    return octl_set_error(ctx, OCTL_E_INVALID, "mask has %lld entries for %lld points",
                          (long long)n, (long long)f->n_ord);
  OCTL_TRY(devbuf_reserve(ctx, f->mask, (size_t)std::max<int64_t>(n, 1)));
  if (n > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(f->mask.p, mask, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  f->mask_valid = true;
  return apply_device_mask(f, n_alive);
}

}  // extern "C"
