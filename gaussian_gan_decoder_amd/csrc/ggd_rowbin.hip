// ggd_rowbin.hip -- two-level stable tile binning (GGD_OPT_BINNING = 3 / auto): the kernels below for tile grids up to 64 x 64,
// ggd_rowbin_wide.inc (same algorithm, bins spread over lane groups) for grids up to 255 x 255.
//
// Contract (stages a6-a8 as a RESULT: per tile, the Gaussians whose rect covers it in
// (depth bits, index) order, plus ranges), from the depth-ordered Gaussians.  The single-level pass there pays O(T) LDS
// work per 1024 Gaussians and writes one lone 4-byte store per (block, tile).  A tile rect is a product of two
// intervals, so the expansion is split into two 1-D counting sorts with <= 64 bins each -- one bin per LANE:
//   level 1 (rows):    Gaussian [y0, y1)  -> one entry {id, x0, x1} in the list of every tile ROW it touches
//   level 2 (columns): row entry [x0, x1) -> the Gaussian id in the list of every TILE of that row it touches
// Both levels are stable (items are consumed in order, chunk by chunk of 1024), so depth order survives and the final lists
// equal the radix-sort path's bit for bit.  A level is three steps:
//   count    per chunk and bin.  Where a kernel does nothing else: an LDS difference array (+1 at lo, -1 at hi, prefix over the
//            lanes) -- atomics are cheaper than the transposes below (see rb_count2_kernel).
//   scan     exclusive prefix over the chunks per bin, bin starts.
//   scatter  a wave turns each round of 64 items into the 64 x 64 item / bin bit matrix and transposes it (wave_cols: lane b then
//            holds the items that cover bin b, in item order, and their popcount is the bin's count); wave_emit walks either
//            the items (a lane keeps its item and looks up {mask, running destination} of every bin it covers in the wave's
//            LDS slab) or the bins (a lane drains its bin, payloads come over by shuffle), whichever is shorter for the round.
//            A chunk's output is staged in LDS in (bin, item) order where it fits and leaves as lane-consecutive runs per bin;
//            entries of one (chunk, bin) are consecutive in memory either way.
// Which kernels take those steps (ggd_launch_rowbin), by what the launches in front have left:
//   counted  folded front end behind the two-launch depth sort (GGD_OPT_L1_COUNTED).  The sort's finish launch stored `packed` and
//            counted the row entries of every bucket and in front of every chunk boundary: rb_level1_counted_kernel sums finished
//            rows and scatters.  Level 2 as on the folded path.  Three launches.
//   folded   the preprocess kernel counted the entries and the instances per row.  rb_level1_kernel: count from the transposes,
//            two-level look-back over the earlier chunks (ggd_lookback.inc), scatter.  Level 2: rb_count2_kernel, then
//            rb_scatter2_kernel<true>, whose workgroups sum the count rows of their tile row's blocks themselves -- no scan launch,
//            no hand-off between workgroups (beyond RB_SCAN_IN_SCATTER_MAX_BLOCKS: level 2 of the plain path).  Three launches.
//   plain    rb_count1 / rb_scan1 (one workgroup) / rb_scatter1 with `packed` between them, rb_count2 / rb_scan2 (one workgroup per
//            tile row; the rows above are summed from their published totals) / rb_scatter2_kernel<false>.  Six launches.
//   wide     grids beyond 64 x 64: the plain path's six launches as rbw_* (ggd_rowbin_wide.inc).
// Stated once and shared: rb_emit_chunk (the emission tail of the three narrow kernels that stage: staging, copy-out, direct form),
// rb_sum_count_rows (16-byte batched row sums: rb_level1_counted_kernel, rb_scatter2_kernel<true>), rb_level1_head (row starts and
// workgroup 0's tables: both one-launch level-1 kernels), rb_write_row_tables, rb_prefix_over_chunks (the four scan kernels), rb_publish_row_sum_above (the two level-2 scans),
// rb_block_row_range, wave_cols / wave_emit (narrow) and wave_cols_w / wave_emit_w (wide).
// Scratch and table layouts, the `packed` record: ggd_binning_layout.h (ggd_rowbin_tmp, RB_TAB_* / RBW_TAB_*, rb_pack_rect).
#include "ggd_common.h"
#include "ggd_lanes.h"

namespace {

#include "ggd_scan.inc"
#include "ggd_lookback.inc"

constexpr int RB_WAVES = RB_THREADS / 64;
constexpr int RB_STAGE = 4096;                     // instances a level-2 workgroup can stage in LDS (16 KB; measured: 4096 / 6144 /
                                                   // 8192 / 12288 -> 3656 / 3640 / 3594 / 3589 frames/s: occupancy beats coverage)
constexpr int RB_STAGE1 = 4096;                    // row entries a level-1 workgroup can stage (32 KB)
constexpr int RB_WCHUNK = 64 * RB_IPL;             // 256 items per wave

// The tables level 2 reads, from the entries per row (lane = row; inc = their inclusive prefix over the lanes): row starts,
// first level-2 block of every row, the rows' published flags cleared (consumed by rb_scan2_kernel, a later launch).
// level-2 blocks cover only the entries that exist in `ent` (ent_cap of them): when a speculative forward
// under-estimated the capacity the rows are clamped, so that counts2 (sized for ent_cap) is never overrun
__device__ __forceinline__ void rb_write_row_tables(uint32_t* tab, int lane, uint32_t tot, uint32_t inc, uint32_t ent_cap) {
  const uint32_t rs = inc - tot;
  tab[RB_TAB_ROWSTART + lane] = rs;
  if (lane == 63) tab[RB_TAB_ROWSTART + 64] = inc;
  const uint32_t have = rs < ent_cap ? min(tot, ent_cap - rs) : 0u;
  const uint32_t nblk = (have + RB_CHUNK - 1) / RB_CHUNK;
  const uint32_t binc = wave_inclusive_scan(nblk);
  tab[RB_TAB_ROWBLK + lane] = binc - nblk;
  if (lane == 63) tab[RB_TAB_ROWBLK + 64] = binc;
  tab[RB_TAB_FLAG + lane] = 0u;
}

// a per-row quantity of the folded front end (lane = row): the sum of its GGD_FOLD_REPS replicas
__device__ __forceinline__ uint32_t rb_fold_sum(const uint32_t* __restrict__ reps, int lane) {
  uint32_t s = 0;
#pragma unroll
  for (int r = 0; r < GGD_FOLD_REPS; ++r) s += reps[r * 64 + lane];
  return s;
}

// The level-1 head of the one-launch kernels: the entries per row (lane = row; tot = rb_fold_sum of the row totals, loaded where the
// caller wants the loads) scanned into row starts; returns the lane's.  The wave that is told to (one wave of workgroup 0) also writes
// the tables level 2 reads and, when given `rowinst`, the instances per row for rb_scatter2_kernel<true> (plain stores: the next
// launch reads them).
__device__ __forceinline__ uint32_t rb_level1_head(uint32_t tot, bool write_tables, uint32_t* __restrict__ tab, uint32_t ent_cap,
                                                   const uint32_t* __restrict__ rowinst) {
  const int lane = threadIdx.x & 63;
  const uint32_t inc = wave_inclusive_scan(tot);
  if (write_tables) {
    rb_write_row_tables(tab, lane, tot, inc, ent_cap);
    if (rowinst) tab[RB_TAB_ROWINST + lane] = rb_fold_sum(rowinst, lane);
  }
  return inc - tot;
}

// Per-bin prefix over chunks (the scan kernels: 16 waves, lane = bin `bin` of count rows `stride` words long): the waves split the
// chunks [c0, c0 + n) evenly and sum their shares, the partial sums meet in part[wave][lane], and every count is replaced by the
// running exclusive prefix of its bin over the chunks.  Returns the bin's total.  (Reusing `part` takes a barrier of the caller's.)
template <int UNROLL>
__device__ __forceinline__ uint32_t rb_prefix_over_chunks(uint32_t* __restrict__ counts, uint32_t c0, uint32_t n, size_t stride,
                                                          int bin, uint32_t (&part)[16][64]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t per = (n + 15u) / 16u;
  const uint32_t b0 = c0 + min(n, (uint32_t)wv * per), b1 = min(c0 + n, b0 + per);
  uint32_t s = 0;
#pragma unroll UNROLL
  for (uint32_t b = b0; b < b1; ++b) s += counts[(size_t)b * stride + bin];
  part[wv][lane] = s;
  __syncthreads();
  uint32_t run = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { const uint32_t p = part[w][lane]; if (w < wv) run += p; tot += p; }
#pragma unroll UNROLL
  for (uint32_t b = b0; b < b1; ++b) {
    const size_t idx = (size_t)b * stride + bin;
    const uint32_t c = counts[idx];
    counts[idx] = run;
    run += c;
  }
  return tot;
}

// ---- level 1 count: rect of every depth-ordered Gaussian (kept, packed, for the scatter) + per-row counts of the chunk
__global__ __launch_bounds__(RB_THREADS) void rb_count1_kernel(const uint2* __restrict__ rect,
                                                               const uint32_t* __restrict__ order,
                                                               const uint32_t* __restrict__ n_vis_ptr, int P,
                                                               uint2* __restrict__ packed, uint32_t* __restrict__ counts1,
                                                               const uint32_t* __restrict__ order_alt,
                                                               const uint32_t* __restrict__ use_alt) {
  __shared__ int diff[65];
  if (use_alt && *use_alt != 0u) order = order_alt;   // the depth sort's last pass was the identity and copied nothing
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint32_t base = (uint32_t)blockIdx.x * RB_CHUNK;
  if (base >= n_vis) return;
  const int tid = threadIdx.x;
  if (tid < 65) diff[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const uint32_t rnk = base + (uint32_t)q * RB_THREADS + tid;
    if (rnk < n_vis) {
      const uint32_t id = order[rnk];
      const uint2 rc = rect[id];   // {minx | maxx << 16, miny | maxy << 16} (grids up to 64 x 64 here)
      const int x0 = (int)(rc.x & 0xffffu), x1 = (int)(rc.x >> 16), y0 = (int)(rc.y & 0xffffu), y1 = (int)(rc.y >> 16);
      const int n = (x1 - x0) * (y1 - y0);
      packed[rnk] = make_uint2(id, n > 0 ? rb_pack_rect((uint32_t)x0, (uint32_t)x1, (uint32_t)y0, (uint32_t)y1) : 0u);
      if (n > 0) { atomicAdd(&diff[y0], 1); atomicAdd(&diff[y1], -1); }
    }
  }
  __syncthreads();
  if (tid < 64) counts1[(size_t)blockIdx.x * 64 + tid] = (uint32_t)wave_inclusive_scan(diff[tid]);
}

// ---- scan over chunks, one workgroup, lane = bin: counts[c][bin] -> exclusive prefix within the bin; totals per bin
//      level 1: rows of one segment (all chunks);   level 2 is handled per row in rb_scan2_kernel.
__global__ __launch_bounds__(1024) void rb_scan1_kernel(uint32_t* __restrict__ counts1,
                                                        const uint32_t* __restrict__ n_vis_ptr, int P,
                                                        uint32_t* __restrict__ tab, uint32_t ent_cap) {
  __shared__ uint32_t part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint32_t tot = rb_prefix_over_chunks<8>(counts1, 0u, (n_vis + RB_CHUNK - 1) / RB_CHUNK, 64, lane, part);
  if (wv == 0) rb_write_row_tables(tab, lane, tot, wave_inclusive_scan(tot), ent_cap);
}

// (wave_transpose64 -- the 64 x 64 item / bin bit matrix across the wave -- is ggd_lanes.h's)

// A wave's items (RB_IPL rounds of 64, lane = item, interval [lo, hi) of bins) against its 64 bins (lane = bin), round 5 form:
//   wave_cols   every round's 64 x 64 item / bin bit matrix, transposed: cols[q] of lane b = the items of round q that cover bin
//               b, in item order.  Returns the lane's (= bin's) number of entries: popcount of its masks -- the counts cost
//               nothing beyond the transposes the emission needs anyway (they used to be an LDS difference array filled with
//               two atomics per item, 25 of rb_scatter2_kernel's 59 us on the head-like scene: same-address LDS atomics
//               serialise).
//   wave_emit   ITEM-parallel: the lane keeps its item and walks the bins b = lo .. hi - 1 it covers; for each it reads
//               {mask of bin b, running destination of bin b} (one 16-byte LDS read from the wave's slab, written by the bin
//               lanes) and stores its payload at destination + (items below it in the mask).  Steps per round = the widest
//               item (a handful), whatever the data; the bin-parallel drain it replaces took as many steps as the fullest bin
//               holds items -- up to 64 where a depth slice of the scene projects onto a few rows (the caps of a shell).
__device__ __forceinline__ uint32_t wave_cols(const uint32_t (&iv)[RB_IPL], int n_items, uint64_t (&cols)[RB_IPL]) {
  uint32_t cnt = 0;
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    cols[q] = 0ull;
    if (q * 64 >= n_items) continue;   // (no `break`: keeps the loop fully unrollable)
    const uint32_t l = iv[q] & 0xffu, h = iv[q] >> 8;
    const uint64_t below_h = h >= 64u ? ~0ull : ((1ull << h) - 1ull);
    const uint64_t row = h > l ? (below_h & ~((1ull << l) - 1ull)) : 0ull;
    cols[q] = wave_transpose64(row);
    cnt += (uint32_t)__popcll(cols[q]);
  }
  return cnt;
}

// Which walk is shorter for this round?  Item-parallel takes as many steps as the widest item has bins, the bin-parallel drain
// as many as the fullest bin has items; both maxima are bracketed with three ballots each (<= 4, 8, 16, more) -- small splats on
// a 64 x 64-tile grid favour the items (and decisively so where a depth slice piles onto a few rows), the wide items of a 4K
// frame the drain (measured with the items only: 4K binning 515 -> 610 us; 1080p 125 -> 117; the 1 M shell 125 -> 88).
__device__ __forceinline__ bool rb_walk_items(uint32_t width, uint32_t fill) {
  const int wi = __ballot(width > 16u) ? 3 : (__ballot(width > 8u) ? 2 : (__ballot(width > 4u) ? 1 : 0));
  const int wf = __ballot(fill > 16u) ? 3 : (__ballot(fill > 8u) ? 2 : (__ballot(fill > 4u) ? 1 : 0));
  return wi <= wf + 1;   // (one LDS read per item step against two cross-lane moves per drain step)
}

template <bool TWO, typename Emit>
__device__ __forceinline__ void wave_emit(const uint32_t (&iv)[RB_IPL], const uint32_t (&pa)[RB_IPL],
                                          const uint32_t (&pb)[RB_IPL], const uint64_t (&cols)[RB_IPL], int n_items,
                                          uint32_t& dst, uint4* slab /* [64], this wave's */, Emit&& emit) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    if (q * 64 >= n_items) continue;
    __builtin_amdgcn_wave_barrier();                      // the previous round's reads of the slab are done (LDS is in order per wave)
    slab[lane] = make_uint4((uint32_t)cols[q], (uint32_t)(cols[q] >> 32), dst, 0u);
    __builtin_amdgcn_wave_barrier();
    const uint32_t l = iv[q] & 0xffu, h = iv[q] >> 8;
    if (rb_walk_items(h > l ? h - l : 0u, (uint32_t)__popcll(cols[q]))) {
      for (uint32_t b = l; __ballot(b < h) != 0ull; ++b) {
        const bool act = b < h;
        const uint4 e = slab[act ? b : 0u];
        const uint64_t m = (uint64_t)e.x | ((uint64_t)e.y << 32);
        if (act) emit(e.z + (uint32_t)__popcll(m & lt_mask), pa[q], TWO ? pb[q] : 0u);
      }
      dst += (uint32_t)__popcll(cols[q]);
    } else {   // bin-parallel drain: the lane (= bin) takes its items lowest first, the payload comes over with ds_bpermute
      uint64_t col = cols[q];
      while (__ballot(col != 0ull) != 0ull) {
        const bool act = col != 0ull;
        const int k = act ? (__ffsll((unsigned long long)col) - 1) : 0;
        col &= col - 1ull;
        const uint32_t a = (uint32_t)__shfl((int)pa[q], k, 64);
        const uint32_t bb = TWO ? (uint32_t)__shfl((int)pb[q], k, 64) : 0u;
        if (act) { emit(dst, a, bb); dst += 1; }
      }
    }
  }
}

// What a chunk emits: a row entry {id, x0 | x1 << 8} at level 1, the Gaussian id at level 2.
struct rb_row_entry {
  using type = uint2;
  static constexpr bool TWO = true;
  static __device__ __forceinline__ uint2 pack(uint32_t id, uint32_t xx) { return make_uint2(id, xx); }
};
struct rb_instance {
  using type = uint32_t;
  static constexpr bool TWO = false;
  static __device__ __forceinline__ uint32_t pack(uint32_t id, uint32_t) { return id; }
};

// The emission tail of a chunk (all four waves; lane = bin): bintot = the chunk's entries per bin, before = those of the earlier
// waves, gbase = where the chunk's run of the bin starts in `out`.  The output is staged in LDS in (bin, item) order and copied out
// with every bin's run as lane-consecutive stores, the bins dealt to the four waves: emitted directly every entry is a lone store
// into one of 64 lists (level 2: 2.2x write amplification, those stores were 15 of rb_scatter2_kernel's 27 us; level 1: the
// head-like scene writes 3.3 M of them).  A chunk with more output than the staging buffer holds keeps the direct form, behind the
// bound check.  `stage` is written below the chunk's own total only, `out` below out_cap only.
template <typename Pay>
__device__ __forceinline__ void rb_emit_chunk(const uint32_t (&iv)[RB_IPL], const uint32_t (&pa)[RB_IPL],
                                              const uint32_t (&pb)[RB_IPL], const uint64_t (&cols)[RB_IPL], int n_items,
                                              uint32_t bintot, uint32_t before, uint32_t gbase, uint4* slab /* [64], this wave's */,
                                              typename Pay::type* stage, uint32_t stage_cap,
                                              typename Pay::type* __restrict__ out, uint32_t out_cap) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t binend = wave_inclusive_scan(bintot);          // same in every wave
  const uint32_t total = wave_pick(binend, 63);
  const uint32_t binbeg = binend - bintot;
  if (total <= stage_cap) {
    uint32_t ldst = binbeg + before;
    wave_emit<Pay::TWO>(iv, pa, pb, cols, n_items, ldst, slab, [&](uint32_t d, uint32_t a, uint32_t b) { stage[d] = Pay::pack(a, b); });
    __syncthreads();
#pragma unroll 4
    for (int c = wv; c < 64; c += RB_WAVES) {
      const uint32_t n = wave_pick(bintot, c);                    // (c is the same in every lane: scalars, as is the loop bound)
      if (n == 0) continue;
      const uint32_t b0 = wave_pick(binbeg, c), g = wave_pick(gbase, c);
      for (uint32_t k = lane; k < n; k += 64) {
        const uint32_t d = g + k;
        if (d < out_cap) out[d] = stage[b0 + k];
      }
    }
    return;
  }
  uint32_t dst = gbase + before;
  wave_emit<Pay::TWO>(iv, pa, pb, cols, n_items, dst, slab, [&](uint32_t d, uint32_t a, uint32_t b) {
    if (d < out_cap) out[d] = Pay::pack(a, b);
  });
}

// Sums n count rows of 64 words over the workgroup: row_of(i) = the address of row i.  16 lanes take a row as four 16-byte columns,
// a wave four rows per load instruction, the rows are dealt to the four waves, and a lane has BATCH = 8 independent loads in flight
// (128 rows per round trip of the workgroup) -- all of a batch requested before any is consumed: these sums sit on the one
// dependent round trip of their kernels, and a load per wait made it n / 16 trips.  The wave's four row groups are folded by
// two lane-block swaps (lane_pair_sum) and lanes 0 - 15 store the wave's partial sums to s_tot[64] (this wave's); BEFORE: those of the rows below `split` to
// s_bef[64] as well.  The caller adds the four waves' partials behind its next barrier.
template <bool BEFORE, typename RowOf>
__device__ __forceinline__ void rb_sum_count_rows(uint32_t n, uint32_t split, RowOf&& row_of, uint32_t* s_tot, uint32_t* s_bef) {
  constexpr int BATCH = 8;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t sub = (uint32_t)lane >> 4, c4 = ((uint32_t)lane & 15u) * 4u;
  uint4 bef4 = make_uint4(0, 0, 0, 0), tot4 = make_uint4(0, 0, 0, 0);
  for (uint32_t k0 = (uint32_t)wv * 4u; k0 < n; k0 += 4u * RB_WAVES * BATCH) {
    uint4 v[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const uint32_t k = k0 + sub + (uint32_t)(4 * RB_WAVES * j);
      v[j] = make_uint4(0, 0, 0, 0);
      if (k < n) v[j] = *reinterpret_cast<const uint4*>(row_of(k) + c4);
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      tot4.x += v[j].x; tot4.y += v[j].y; tot4.z += v[j].z; tot4.w += v[j].w;
      if constexpr (BEFORE) {
        const uint32_t k = k0 + sub + (uint32_t)(4 * RB_WAVES * j);
        const uint32_t m = k < split ? 0xffffffffu : 0u;
        bef4.x += v[j].x & m; bef4.y += v[j].y & m; bef4.z += v[j].z & m; bef4.w += v[j].w & m;
      }
    }
  }
  auto fold4 = [](uint4& v) {   // the wave's four row groups hold the same columns
    v.x = lane_pair_sum<32>(lane_pair_sum<16>(v.x)); v.y = lane_pair_sum<32>(lane_pair_sum<16>(v.y));
    v.z = lane_pair_sum<32>(lane_pair_sum<16>(v.z)); v.w = lane_pair_sum<32>(lane_pair_sum<16>(v.w));
  };
  fold4(tot4);
  if constexpr (BEFORE) fold4(bef4);
  if (lane < 16) {
    if constexpr (BEFORE) *reinterpret_cast<uint4*>(&s_bef[c4]) = bef4;
    *reinterpret_cast<uint4*>(&s_tot[c4]) = tot4;
  }
}

// ---- level 1 scatter: {id, x0 | x1 << 8} into the list of every row in [y0, y1)
__global__ __launch_bounds__(RB_THREADS) void rb_scatter1_kernel(const uint2* __restrict__ packed,
                                                                 const uint32_t* __restrict__ n_vis_ptr, int P,
                                                                 const uint32_t* __restrict__ prefix1,
                                                                 const uint32_t* __restrict__ tab,
                                                                 uint2* __restrict__ ent, uint32_t ent_cap) {
  __shared__ uint4 slab[RB_WAVES][64];
  __shared__ uint32_t wcnt[RB_WAVES][64];
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint32_t base = (uint32_t)blockIdx.x * RB_CHUNK;
  if (base >= n_vis) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t wbeg = base + (uint32_t)wv * RB_WCHUNK;
  const int n_items = (int)min((uint32_t)RB_WCHUNK, n_vis > wbeg ? n_vis - wbeg : 0u);
  uint32_t iv[RB_IPL], pa[RB_IPL], pb[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const int i = q * 64 + lane;
    uint2 it = make_uint2(0, 0);
    if (i < n_items) it = packed[wbeg + i];
    pa[q] = it.x; pb[q] = rb_packed_cols(it.y);
    iv[q] = rb_packed_rows(it.y);
  }
  uint64_t cols[RB_IPL];
  const uint32_t mine = wave_cols(iv, n_items, cols);
  wcnt[wv][lane] = mine;
  __syncthreads();
  uint32_t dst = tab[RB_TAB_ROWSTART + lane] + prefix1[(size_t)blockIdx.x * 64 + lane];
#pragma unroll
  for (int w = 0; w < RB_WAVES; ++w) if (w < wv) dst += wcnt[w][lane];
  wave_emit<true>(iv, pa, pb, cols, n_items, dst, slab[wv], [&](uint32_t d, uint32_t id, uint32_t xx) {
    if (d < ent_cap) ent[d] = make_uint2(id, xx);
  });
}

// ---- level 1 in ONE launch (folded front end: the entries per row were counted by the preprocess kernel, GGD_FOLD_ROWTOT):
//      count, two-level look-back over the earlier chunks (lane = row; status words [chunk][64] then [group][64], zero at
//      launch -- lookback_two_level, as the depth sort's passes), scatter.  Replaces rb_count1 / rb_scan1 /
//      rb_scatter1 and the `packed` round trip between them.  Every workgroup derives the row starts from the 64 x REPS row
//      totals itself; workgroup 0 also writes the tables level 2 reads.  Workgroups wait only for lower-numbered ones, which
//      the dispatcher started earlier.
__global__ __launch_bounds__(RB_THREADS) void rb_level1_kernel(const uint2* __restrict__ rect, const uint32_t* __restrict__ order,
                                                               const uint32_t* __restrict__ n_vis_ptr, int P,
                                                               const uint32_t* __restrict__ rowtot, uint32_t* status,
                                                               int chunks_max, int gshift_max, uint32_t* __restrict__ tab,
                                                               uint2* __restrict__ ent, uint32_t ent_cap,
                                                               const uint32_t* __restrict__ order_alt,
                                                               const uint32_t* __restrict__ use_alt,
                                                               const uint32_t* __restrict__ rowinst) {
  __shared__ uint4 slab[RB_WAVES][64];
  __shared__ uint32_t wcnt[RB_WAVES][64];
  __shared__ uint32_t s_base[64];
  __shared__ uint2 stage[RB_STAGE1];
  if (use_alt && *use_alt != 0u) order = order_alt;   // the depth sort's last pass was the identity and copied nothing
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t rowstart = 0;
  if (wv == 0) rowstart = rb_level1_head(rb_fold_sum(rowtot, lane), blockIdx.x == 0, tab, ent_cap, rowinst);
  const uint32_t base = (uint32_t)blockIdx.x * RB_CHUNK;
  if (base >= n_vis) return;
  const uint32_t wbeg = base + (uint32_t)wv * RB_WCHUNK;
  const int n_items = (int)min((uint32_t)RB_WCHUNK, n_vis > wbeg ? n_vis - wbeg : 0u);
  uint32_t iv[RB_IPL], pa[RB_IPL], pb[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const int i = q * 64 + lane;
    pa[q] = 0; pb[q] = 0; iv[q] = 0;
    if (i < n_items) {
      const uint32_t id = order[wbeg + i];
      const uint2 rc = rect[id];   // {minx | maxx << 16, miny | maxy << 16}
      const uint32_t x0 = rc.x & 0xffffu, x1 = rc.x >> 16, y0 = rc.y & 0xffffu, y1 = rc.y >> 16;
      pa[q] = id;
      if ((int)(x1 - x0) * (int)(y1 - y0) > 0) { pb[q] = x0 | (x1 << 8); iv[q] = y0 | (y1 << 8); }
    }
  }
  uint64_t cols[RB_IPL];
  const uint32_t mine = wave_cols(iv, n_items, cols);
  wcnt[wv][lane] = mine;
  __syncthreads();
  if (wv == 0) {
    const uint32_t local = wcnt[0][lane] + wcnt[1][lane] + wcnt[2][lane] + wcnt[3][lane];
    const int chunk = (int)blockIdx.x;
    const int live = (int)((n_vis + RB_CHUNK - 1) / RB_CHUNK);   // group size ~ sqrt(live chunks), never above the launch's
    const int gs = min(ggd_group_shift(live), gshift_max);
    s_base[lane] = lookback_two_level<64>(status, lane, chunks_max, chunk, gs, local, rowstart);
  }
  __syncthreads();
  uint32_t before = 0, rowtot_c = 0;   // lane = row: this chunk's entries of the earlier waves / of the whole chunk
#pragma unroll
  for (int w = 0; w < RB_WAVES; ++w) { const uint32_t c = wcnt[w][lane]; if (w < wv) before += c; rowtot_c += c; }
  rb_emit_chunk<rb_row_entry>(iv, pa, pb, cols, n_items, rowtot_c, before, s_base[lane], slab[wv], stage, RB_STAGE1, ent, ent_cap);
}

// ---- level 1 behind the two-launch depth sort (GGD_OPT_L1_COUNTED): rb_level1_kernel without the look-back.  The sort's finish
//      launch left, by plain stores (msd_bucket_rows, ggd_msd_finish.inc): packed[rank] = {id, rect}, bucket_rows[b][row] = the row
//      entries of bucket b, boundary_rows[k][row] = those of the elements in front of rank 1024 k inside the bucket that holds
//      it.  Chunk k starts in row r at
//        row start[r] + sum of bucket_rows[b'][r] over the buckets b' that lie wholly in front of rank 1024 k + boundary_rows[k][r]
//      -- every term is final when this launch starts; no workgroup waits for another, no status words, no atomics.
//      Two round trips: {bucket histogram, row totals, kept count, the chunk's packed items, its boundary row}, then the bucket rows
//      (rb_sum_count_rows); behind them the shared emission tail, rb_emit_chunk.  A bucket counts when it is non-empty (an empty one
//      has no workgroup that writes its row) and ends at or below rank 1024 k; which those are follows from the histogram's prefix.
//      A frame the front end's verdict fails (a key outside the window, clamped into the last
//      bucket; a bucket above GGD_MSD_CAP, left in index order) has complete tables too: the lists are those of the order the sort left.
//      Bounds: items are read at min(rank, P - 1); rows unpacked from `packed` are clamped to 64; bucket indices come from the
//      1024-word histogram; k < gridDim = the rows boundary_rows has; ent is written below ent_cap only, the staging buffer below
//      the chunk's own total.
__global__ __launch_bounds__(RB_THREADS) void rb_level1_counted_kernel(const uint2* __restrict__ packed,
                                                                       const uint32_t* __restrict__ hist /* [GGD_MSD_BINS] */,
                                                                       const uint32_t* __restrict__ n_vis_ptr, int P,
                                                                       const uint32_t* __restrict__ rowtot,
                                                                       const uint32_t* __restrict__ bucket_rows,
                                                                       const uint32_t* __restrict__ boundary_rows,
                                                                       uint32_t* __restrict__ tab, uint2* __restrict__ ent,
                                                                       uint32_t ent_cap, const uint32_t* __restrict__ rowinst) {
  __shared__ uint4 slab[RB_WAVES][64];
  __shared__ uint32_t wcnt[RB_WAVES][64];
  __shared__ uint2 stage[RB_STAGE1];
  __shared__ uint32_t s_scan[RB_WAVES][2];
  __shared__ __attribute__((aligned(16))) uint32_t s_rows[RB_WAVES][64];         // the waves' partial sums of their bucket rows
  // the buckets in front of the chunk that count: in the staging buffer, which is first written behind the barrier that follows
  // their last use (with them in LDS of their own the kernel fell from four workgroups a CU to three)
  uint16_t* s_used = reinterpret_cast<uint16_t*>(stage);
  static_assert(GGD_MSD_BINS * sizeof(uint16_t) <= sizeof(stage), "the bucket list fits the staging buffer");
  static_assert(GGD_MSD_BINS == 4 * RB_THREADS, "a thread takes four buckets of the histogram");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t base = (uint32_t)blockIdx.x * RB_CHUNK;
  const uint32_t wbeg = base + (uint32_t)wv * RB_WCHUNK;
  // first round trip: nothing below depends on another load's value
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint4 h4 = reinterpret_cast<const uint4*>(hist)[tid];
  const uint32_t tot = rb_fold_sum(rowtot, lane);
  const uint32_t bound = boundary_rows[(size_t)blockIdx.x * 64 + lane];
  uint2 raw[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) raw[q] = packed[min(wbeg + (uint32_t)(q * 64 + lane), (uint32_t)P - 1u)];
  const uint32_t rowstart = rb_level1_head(tot, blockIdx.x == 0 && wv == 0, tab, ent_cap, rowinst);
  if (base >= n_vis) return;
  const int n_items = (int)min((uint32_t)RB_WCHUNK, n_vis > wbeg ? n_vis - wbeg : 0u);
  // the buckets that end at or below `base`: thread t holds buckets 4 t .. 4 t + 3; one scan carries their sizes and their number
  uint32_t n_used;
  {
    const uint32_t h[4] = {h4.x, h4.y, h4.z, h4.w};
    const uint32_t hsum = h4.x + h4.y + h4.z + h4.w;
    const uint32_t hinc = wave_inclusive_scan(hsum);
    if (lane == 63) s_scan[wv][0] = hinc;
    __syncthreads();
    uint32_t end = hinc - hsum;   // keys in front of bucket 4 t
#pragma unroll
    for (int w = 0; w < RB_WAVES; ++w) if (w < wv) end += s_scan[w][0];
    uint32_t use = 0;             // bit j: bucket 4 t + j counts
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      end += h[j];
      if (h[j] != 0u && end <= base) use |= 1u << j;
    }
    const uint32_t ucnt = (uint32_t)__popc(use);
    const uint32_t uinc = wave_inclusive_scan(ucnt);
    if (lane == 63) s_scan[wv][1] = uinc;
    __syncthreads();
    uint32_t pos = uinc - ucnt;
    n_used = 0;
#pragma unroll
    for (int w = 0; w < RB_WAVES; ++w) { const uint32_t c = s_scan[w][1]; if (w < wv) pos += c; n_used += c; }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (use & (1u << j)) s_used[pos++] = (uint16_t)(4 * tid + j);   // pos < n_used <= GGD_MSD_BINS
  }
  uint32_t iv[RB_IPL], pa[RB_IPL], pb[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const bool have = q * 64 + lane < n_items;
    const uint32_t y0 = min(rb_packed_y0(raw[q].y), 64u), y1 = min(rb_packed_y1(raw[q].y), 64u);
    pa[q] = have ? raw[q].x : 0u;
    pb[q] = have ? rb_packed_cols(raw[q].y) : 0u;
    iv[q] = have ? y0 | (y1 << 8) : 0u;
  }
  uint64_t cols[RB_IPL];
  const uint32_t mine = wave_cols(iv, n_items, cols);
  wcnt[wv][lane] = mine;
  __syncthreads();   // s_used is complete (and wcnt, for the barrier below to publish with s_rows)
  // second (and last) round trip: the rows of the buckets in front
  rb_sum_count_rows<false>(n_used, 0u, [&](uint32_t i) { return bucket_rows + (size_t)s_used[i] * 64; }, s_rows[wv], nullptr);
  __syncthreads();
  uint32_t before = 0, rowtot_c = 0;   // lane = row: this chunk's entries of the earlier waves / of the whole chunk
#pragma unroll
  for (int w = 0; w < RB_WAVES; ++w) { const uint32_t c = wcnt[w][lane]; if (w < wv) before += c; rowtot_c += c; }
  const uint32_t gbase = rowstart + bound + s_rows[0][lane] + s_rows[1][lane] + s_rows[2][lane] + s_rows[3][lane];
  rb_emit_chunk<rb_row_entry>(iv, pa, pb, cols, n_items, rowtot_c, before, gbase, slab[wv], stage, RB_STAGE1, ent, ent_cap);
}

// level-2 block -> (row, chunk within the row)
// (one load per lane + a ballot: a binary search over the table is six DEPENDENT global loads, which was most of a
// level-2 workgroup's lifetime)
// ... and the row's entry range with it: the block table and the row starts are requested TOGETHER (a level-2 workgroup is a
// chain of dependent memory round trips at full occupancy -- block table -> row start -> entries -> tile starts was four of
// them; this form makes it two: {block table, row starts}, then {entries, tile starts, chunk prefixes})
__device__ __forceinline__ bool rb_block_row_range(const uint32_t* __restrict__ tab, uint32_t blk, uint32_t ent_cap, int& row,
                                                   uint32_t& chunk, uint32_t& rbeg, uint32_t& rend) {
  const int lane = threadIdx.x & 63;
  const uint32_t first = tab[RB_TAB_ROWBLK + lane];
  const uint32_t total = tab[RB_TAB_ROWBLK + 64];
  const uint32_t start = tab[RB_TAB_ROWSTART + lane];
  const uint32_t all = tab[RB_TAB_ROWSTART + 64];
  if (blk >= total) return false;
  const int r = __popcll(__ballot(first <= blk)) - 1;
  row = r; chunk = blk - wave_pick(first, r);
  rbeg = wave_pick(start, r);
  rend = min(r == 63 ? all : wave_pick(start, (r + 1) & 63), ent_cap);
  return true;
}

// (counts by an LDS difference array here: the kernel does nothing else, and four bit-matrix transposes per wave -- the form the
// scatter kernels take their counts from, where the emission needs the transposes anyway -- cost more than the atomics:
// measured 7.7 vs 4.8 us on the 1 M cube scene, 14.7 vs 9.0 us on the shell)
__global__ __launch_bounds__(RB_THREADS) void rb_count2_kernel(const uint2* __restrict__ ent, uint32_t ent_cap,
                                                               const uint32_t* __restrict__ tab,
                                                               uint32_t* __restrict__ counts2) {
  __shared__ int diff[65];
  int row; uint32_t chunk, rbeg, rend;
  if (!rb_block_row_range(tab, blockIdx.x, ent_cap, row, chunk, rbeg, rend)) return;
  const int tid = threadIdx.x;
  const uint32_t base = rbeg + chunk * RB_CHUNK;
  uint32_t xs[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {       // (requested before the barrier below)
    const uint32_t i = base + (uint32_t)q * RB_THREADS + tid;
    xs[q] = i < rend ? ent[i].y : 0u;
  }
  if (tid < 65) diff[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const uint32_t x0 = xs[q] & 0xffu, x1 = (xs[q] >> 8) & 0xffu;
    if (x1 > x0) { atomicAdd(&diff[x0], 1); atomicAdd(&diff[x1], -1); }
  }
  __syncthreads();
  if (tid < 64) counts2[(size_t)blockIdx.x * 64 + tid] = (uint32_t)wave_inclusive_scan(diff[tid]);
}

// Wave 0 of the scan workgroup of tile row r: publishes the row's instances (`mine`, taken from lane 63; release) and returns those
// of the rows above, summed from their published totals (relaxed poll, one acquire).  inst / flag: the tables' [row] words.
__device__ __forceinline__ uint32_t rb_publish_row_sum_above(uint32_t* inst, uint32_t* flag, int r, uint32_t mine) {
  const int lane = threadIdx.x & 63;
  if (lane == 63) {
    inst[r] = mine;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __hip_atomic_store(&flag[r], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int rr = lane; rr < r; rr += 64)
    while (__hip_atomic_load(&flag[rr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {}
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  uint32_t above = 0;
  for (int rr = lane; rr < r; rr += 64) above += __hip_atomic_load(&inst[rr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return wave_sum_to_all(above);
}

// ---- level-2 scan, one workgroup per tile row: exclusive prefix over the row's chunks (lane = column, 16 waves split
//      the chunks), tile totals, then the start of every tile list.  The only cross-row quantity is the number of
//      instances in the rows above: every workgroup publishes its row total (release) and sums the totals of the lower
//      rows (relaxed poll + acquire).  Workgroups only ever wait for lower-numbered ones.
__global__ __launch_bounds__(1024) void rb_scan2_kernel(uint32_t* __restrict__ counts2, uint32_t* tab, int gx, int gy,
                                                        uint32_t* __restrict__ ranges) {
  __shared__ uint32_t part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x;
  const uint32_t b0 = tab[RB_TAB_ROWBLK + r], b1 = tab[RB_TAB_ROWBLK + r + 1];
  const uint32_t tot = rb_prefix_over_chunks<4>(counts2, b0, b1 - b0, 64, lane, part);
  if (wv == 0) {
    const uint32_t inc = wave_inclusive_scan(tot);
    const uint32_t rowbase = rb_publish_row_sum_above(tab + RB_TAB_ROWINST, tab + RB_TAB_FLAG, r, inc);
    if (lane < gx) {
      const uint32_t start = rowbase + inc - tot;
      tab[RB_TAB_TILESTART + r * 64 + lane] = start;
      const int t = r * gx + lane;
      ranges[2 * t] = tot ? start : 0u;
      ranges[2 * t + 1] = tot ? start + tot : 0u;
    }
  }
}

// SCAN (folded front end; no rb_scan2_kernel in front): counts2 holds rb_count2_kernel's RAW counts and tab[RB_TAB_ROWINST] the
// instances per row as the preprocess kernel counted them.  The workgroup of block (row r, chunk c) forms its tile starts itself:
//   start(r, col) = instances of the rows above r + exclusive prefix over the columns of total[col] + before[col],
//   total / before = sum of counts2[b][col] over all blocks b of row r / over the blocks in front of chunk c
// -- the count rows of the row's blocks (rb_sum_count_rows) are requested in the same round trip as the entries, and the waves'
// partial sums meet at the barrier behind wave_cols.  Nothing is handed from one workgroup to another (the two forms that did, profiles/REJECTED.md round 5, doubled
// rb_count2_kernel).
// Chunk 0 of a row writes the row's ranges; a row without blocks has no workgroup, so workgroup z < gy writes the zero ranges of
// row z when that row has none.  The reads grow with the square of a row's blocks: RB_SCAN_IN_SCATTER_MAX_BLOCKS.
template <bool SCAN>
__global__ __launch_bounds__(RB_THREADS) void rb_scatter2_kernel(const uint2* __restrict__ ent, uint32_t ent_cap,
                                                                 const uint32_t* __restrict__ tab,
                                                                 const uint32_t* __restrict__ prefix2,
                                                                 uint32_t* __restrict__ list, uint32_t capacity,
                                                                 uint32_t main_blocks, ggd_scan_piggy pg, int gx, int gy,
                                                                 uint32_t* __restrict__ ranges) {
  __shared__ uint4 slab[RB_WAVES][64];
  __shared__ uint32_t wcnt[RB_WAVES][64];
  __shared__ __attribute__((aligned(16))) uint32_t wsum[SCAN ? 2 * RB_WAVES : 1][64];   // SCAN: the waves' partial {before, total} per column
  __shared__ uint32_t stage[RB_STAGE];
  if (blockIdx.x >= main_blocks) {   // appended workgroups: last step of the offsets scan (see ggd_scan_piggy)
    scan_apply_block(pg.in, pg.out, pg.n, pg.block_sums, (int)(blockIdx.x - main_blocks), stage, pg.sum_stride);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t rowinst = 0, rowblks = 0;   // lane = row: its instances, its level-2 blocks
  if constexpr (SCAN) {   // (first round trip, with rb_block_row_range's four loads)
    rowinst = tab[RB_TAB_ROWINST + lane];
    rowblks = tab[RB_TAB_ROWBLK + lane + 1] - tab[RB_TAB_ROWBLK + lane];
    if ((int)blockIdx.x < gy && wv == 0) {
      const uint32_t nb_z = wave_pick(rowblks, (int)blockIdx.x);
      if (nb_z == 0u && lane < gx) {
        const int t = (int)blockIdx.x * gx + lane;
        ranges[2 * t] = 0u;
        ranges[2 * t + 1] = 0u;
      }
    }
  }
  int row; uint32_t chunk, rbeg, rend;
  if (!rb_block_row_range(tab, blockIdx.x, ent_cap, row, chunk, rbeg, rend)) return;
  const uint32_t wbeg = rbeg + chunk * RB_CHUNK + (uint32_t)wv * RB_WCHUNK;
  const int n_items = (int)min((uint32_t)RB_WCHUNK, rend > wbeg ? rend - wbeg : 0u);
  uint32_t iv[RB_IPL], pa[RB_IPL], pb[RB_IPL];
  // second (and last) round trip: the entries, the tile starts and the chunk's prefixes (SCAN: the count rows of the row's blocks),
  // all requested before anything waits.  (A lane without an item reads the block's first entry, which exists: behind
  // `if (i < n_items)` every one of the four loads was followed by its own wait -- four round trips instead of one.)
  const uint32_t blkbeg = rbeg + chunk * RB_CHUNK;
  uint2 raw[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const int i = q * 64 + lane;
    raw[q] = ent[i < n_items ? wbeg + (uint32_t)i : blkbeg];
  }
  uint32_t gbase = 0;
  if constexpr (SCAN) {
    const uint32_t blk0 = blockIdx.x - chunk;                                        // first block of the row
    const uint32_t nblk_row = wave_pick(rowblks, row);                               // >= chunk + 1
    // (the cube's 19 blocks a row, the shell's 50 - 130 are one batch of rb_sum_count_rows)
    rb_sum_count_rows<true>(nblk_row, chunk, [&](uint32_t k) { return prefix2 + (size_t)(blk0 + k) * 64; }, wsum[RB_WAVES + wv], wsum[wv]);
  } else {
    gbase = tab[RB_TAB_TILESTART + row * 64 + lane] + prefix2[(size_t)blockIdx.x * 64 + lane];
  }
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {   // (the entries are looked at only here, behind the other requests)
    const bool have = q * 64 + lane < n_items;
    pa[q] = have ? raw[q].x : 0u; pb[q] = 0;
    iv[q] = have ? raw[q].y & 0xffffu : 0u;   // x0 | x1 << 8
  }
  uint64_t cols[RB_IPL];
  const uint32_t mine = wave_cols(iv, n_items, cols);
  wcnt[wv][lane] = mine;
  __syncthreads();
  if constexpr (SCAN) {
    uint32_t bef = 0, tot = 0;   // lane = column: instances of the row's earlier blocks / of the whole row
#pragma unroll
    for (int w = 0; w < RB_WAVES; ++w) { bef += wsum[w][lane]; tot += wsum[RB_WAVES + w][lane]; }
    const uint32_t rinc = wave_inclusive_scan(rowinst);
    const uint32_t rowbase = wave_pick(rinc - rowinst, row);                         // instances of the rows above
    const uint32_t start = rowbase + wave_inclusive_scan(tot) - tot;
    gbase = start + bef;
    if (chunk == 0u && wv == 0 && lane < gx) {
      const int t = row * gx + lane;
      ranges[2 * t] = tot ? start : 0u;
      ranges[2 * t + 1] = tot ? start + tot : 0u;
    }
  }
  uint32_t before = 0, coltot = 0;   // lane = column: instances of the earlier waves / of the whole chunk
#pragma unroll
  for (int w = 0; w < RB_WAVES; ++w) { const uint32_t c = wcnt[w][lane]; if (w < wv) before += c; coltot += c; }
  rb_emit_chunk<rb_instance>(iv, pa, pb, cols, n_items, coltot, before, gbase, slab[wv], stage, RB_STAGE, list, capacity);
}

#include "ggd_rowbin_wide.inc"

// ---- self-test of ggd_lanes.h (ggd_selftest_lanes): one wave per 64 input words; lane l takes in[64 w + l] (x = its low word) and
//      writes GGD_LANES_SELFTEST_WORDS words: every primitive next to the __shfl form it replaced, for the test to compare both with
//      its own arithmetic.  Layout (ggd_raster.h): {new, shfl} pairs of scan (uint32), scan (int), sum, max; lane_xor<1 .. 32> new,
//      then shfl; wave_pick of every lane new, then shfl; transpose {lo, hi} new, then shfl.
namespace lanes_shfl {
template <typename T>
__device__ __forceinline__ T scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
template <int D, uint32_t M>
__device__ __forceinline__ void tr_stage(uint32_t& lo, uint32_t& hi, uint32_t lane) {
  const bool up = (lane & (uint32_t)D) != 0;
  const uint32_t keep = up ? ~M : M;
  const uint32_t slo = up ? ((lo & M) << D) : ((lo & ~M) >> D);
  const uint32_t shi = up ? ((hi & M) << D) : ((hi & ~M) >> D);
  lo = (lo & keep) | (uint32_t)__shfl_xor((int)slo, D, 64);
  hi = (hi & keep) | (uint32_t)__shfl_xor((int)shi, D, 64);
}
__device__ __forceinline__ uint64_t transpose64(uint64_t row) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t lo = (uint32_t)row, hi = (uint32_t)(row >> 32);
  {
    const bool up = (lane & 32u) != 0;
    const uint32_t recv = (uint32_t)__shfl_xor((int)(up ? lo : hi), 32, 64);
    if (up) lo = recv; else hi = recv;
  }
  tr_stage<16, 0x0000FFFFu>(lo, hi, lane);
  tr_stage<8, 0x00FF00FFu>(lo, hi, lane);
  tr_stage<4, 0x0F0F0F0Fu>(lo, hi, lane);
  tr_stage<2, 0x33333333u>(lo, hi, lane);
  tr_stage<1, 0x55555555u>(lo, hi, lane);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
}  // namespace lanes_shfl

__global__ __launch_bounds__(64) void selftest_lanes_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  const uint64_t row = in[(size_t)blockIdx.x * 64 + lane];
  const uint32_t x = (uint32_t)row;
  uint32_t* o = out + ((size_t)blockIdx.x * 64 + lane) * GGD_LANES_SELFTEST_WORDS;
  o[0] = wave_inclusive_scan(x);                 o[1] = lanes_shfl::scan(x);
  o[2] = (uint32_t)wave_inclusive_scan((int)x);  o[3] = (uint32_t)lanes_shfl::scan((int)x);
  o[4] = wave_sum_to_all(x);                     o[5] = (uint32_t)__shfl((int)lanes_shfl::scan(x), 63, 64);
  uint32_t m = x;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, sh, 64));
  o[6] = wave_max_to_all(x);                     o[7] = m;
  o[8] = lane_xor<1>(x);   o[9] = lane_xor<2>(x);   o[10] = lane_xor<4>(x);
  o[11] = lane_xor<8>(x);  o[12] = lane_xor<16>(x); o[13] = lane_xor<32>(x);
#pragma unroll
  for (int k = 0; k < 6; ++k) o[14 + k] = (uint32_t)__shfl_xor((int)x, 1 << k, 64);
#pragma unroll 1
  for (int c = 0; c < 64; ++c) {
    o[20 + c] = wave_pick(x, c);
    o[84 + c] = (uint32_t)__shfl((int)x, c, 64);
  }
  const uint64_t tn = wave_transpose64(row), ts = lanes_shfl::transpose64(row);
  o[148] = (uint32_t)tn; o[149] = (uint32_t)(tn >> 32);
  o[150] = (uint32_t)ts; o[151] = (uint32_t)(ts >> 32);
  o[152] = lane_pair_sum<16>(x); o[153] = lane_pair_sum<32>(x);
  o[154] = wave_max_lane63(x);   o[155] = wave_sum_lane63(x);
}
static_assert(GGD_LANES_SELFTEST_WORDS == 156, "selftest_lanes_kernel's layout");

}  // namespace

int ggd_launch_selftest_lanes(ggd_ctx* ctx, hipStream_t s, const uint64_t* in, uint32_t* out, int n_waves) {
  selftest_lanes_kernel<<<n_waves, 64, 0, s>>>(in, out);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

// grids up to 64 x 64 tiles: the lane-per-bin kernels above; up to 255 x 255: ggd_rowbin_wide.inc
bool ggd_rowbin_supported(int W, int H) { return W > 0 && H > 0 && (W + 15) / 16 <= 255 && (H + 15) / 16 <= 255; }

static int rb_launch_status(ggd_ctx* ctx) {   // the launches above, as a return code
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

// capacity: upper bound on num_rendered (the level-1 entry count is <= num_rendered); order = depth-sorted ids.
ggd_rowbin_result ggd_launch_rowbin(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const uint2* rect, const uint32_t* order,
                                    const uint32_t* n_vis_ptr, uint32_t* list, uint32_t* ranges, uint32_t capacity, void* tmp,
                                    size_t tmp_bytes, const ggd_rowbin_opts& opts) {
  const ggd_scan_piggy* apply = opts.apply;
  const auto& fold = opts.fold;
  if (!ggd_rowbin_supported(prm.width, prm.height)) return {ggd_fail(ctx, GGD_E_INVALID, "tile grid too large for row binning")};
  const ggd_rowbin_tmp lay = ggd_rowbin_layout(prm.P, capacity, prm.width, prm.height);
  if (tmp_bytes < lay.total) return {ggd_fail(ctx, GGD_E_INVALID, "rowbin tmp too small")};
  const int gx = (prm.width + 15) / 16, gy = (prm.height + 15) / 16;
  const bool wide = rb_is_wide(prm.width, prm.height);
  char* p = static_cast<char*>(tmp);
  uint2* packed = reinterpret_cast<uint2*>(p + lay.packed);
  uint32_t* counts1 = reinterpret_cast<uint32_t*>(p + lay.counts1);
  uint32_t* tab = reinterpret_cast<uint32_t*>(p + lay.tab);
  uint2* ent = reinterpret_cast<uint2*>(p + lay.ent);
  uint32_t* counts2 = reinterpret_cast<uint32_t*>(p + lay.counts2);
  const int nb1 = rb_blocks1(prm.P);
  const uint32_t nb2 = rb_blocks2(capacity, wide);
  const uint32_t nb_apply = apply ? (uint32_t)apply->nb : 0u;   // step 3 of a riding scan, appended to the last launch
  const ggd_scan_piggy pg = apply ? *apply : ggd_scan_piggy{};
  static_assert(RB_THREADS == SCAN_THREADS, "the appended scan workgroups share the launch's block size");
  if (wide) {
    const int ngy = (gy + 63) / 64, ngx = (gx + 63) / 64, nby = 64 * ngy, nbx = 64 * ngx;
    hipLaunchKernelGGL(rbw_count1_kernel, dim3(nb1), dim3(RB_THREADS), 0, s, rect, order, n_vis_ptr, prm.P, nby, packed,
                       counts1, opts.order_alt, opts.use_alt);
    hipLaunchKernelGGL(rbw_scan1_kernel, dim3(1), dim3(1024), 0, s, counts1, n_vis_ptr, prm.P, ngy, tab, capacity);
    hipLaunchKernelGGL(rbw_scatter1_kernel, dim3(nb1), dim3(RB_THREADS), 0, s, packed, n_vis_ptr, prm.P, ngy, counts1, tab,
                       ent, capacity);
    hipLaunchKernelGGL(rbw_count2_kernel, dim3(nb2), dim3(RB_THREADS), 0, s, ent, capacity, tab, nbx, counts2);
    hipLaunchKernelGGL(rbw_scan2_kernel, dim3(gy), dim3(1024), 0, s, counts2, tab, gx, gy, ngx, ranges);
    hipLaunchKernelGGL(rbw_scatter2_kernel, dim3(nb2 + nb_apply), dim3(RB_THREADS), 0, s, ent, capacity, tab, ngx, counts2, list,
                       capacity, nb2, pg);
    return {rb_launch_status(ctx)};
  }
  // the front end counted the instances per row as well: level 2 needs no scan launch (up to the block count the quadratic
  // reads of rb_scatter2_kernel<true> are admitted for)
  const bool fused2 = fold.rowtot && fold.status1 && fold.rowinst && nb2 <= RB_SCAN_IN_SCATTER_MAX_BLOCKS;
  if (opts.counted_hist) {
    // the two-launch sort's finish kernel left packed / bucket_rows / boundary_rows (ggd_rowbin_counted) and opts.counted_hist is the
    // bucket histogram it read: level 1 without the look-back
    if (!fold.rowtot || tmp_bytes < lay.total_counted) return {ggd_fail(ctx, GGD_E_INVALID, "rowbin: counted level 1 needs the folded front end and its row tables")};
    hipLaunchKernelGGL(rb_level1_counted_kernel, dim3(nb1), dim3(RB_THREADS), 0, s, packed, opts.counted_hist, n_vis_ptr, prm.P,
                       fold.rowtot, reinterpret_cast<const uint32_t*>(p + lay.bucket_rows),
                       reinterpret_cast<const uint32_t*>(p + lay.boundary_rows), tab, ent, capacity, fused2 ? fold.rowinst : nullptr);
  } else if (fold.rowtot && fold.status1) {   // (the group words were laid out for ggd_group_shift(chunks): ggd_fold_ctl_words)
    hipLaunchKernelGGL(rb_level1_kernel, dim3(nb1), dim3(RB_THREADS), 0, s, rect, order, n_vis_ptr, prm.P, fold.rowtot,
                       fold.status1, nb1, ggd_group_shift(nb1), tab, ent, capacity, opts.order_alt, opts.use_alt,
                       fused2 ? fold.rowinst : nullptr);
  } else {
    hipLaunchKernelGGL(rb_count1_kernel, dim3(nb1), dim3(RB_THREADS), 0, s, rect, order, n_vis_ptr, prm.P, packed, counts1,
                       opts.order_alt, opts.use_alt);
    hipLaunchKernelGGL(rb_scan1_kernel, dim3(1), dim3(1024), 0, s, counts1, n_vis_ptr, prm.P, tab, capacity);
    hipLaunchKernelGGL(rb_scatter1_kernel, dim3(nb1), dim3(RB_THREADS), 0, s, packed, n_vis_ptr, prm.P, counts1, tab,
                       ent, capacity);
  }
  hipLaunchKernelGGL(rb_count2_kernel, dim3(nb2), dim3(RB_THREADS), 0, s, ent, capacity, tab, counts2);
  if (fused2) {
    hipLaunchKernelGGL(rb_scatter2_kernel<true>, dim3(nb2 + nb_apply), dim3(RB_THREADS), 0, s, ent, capacity, tab, counts2, list,
                       capacity, nb2, pg, gx, gy, ranges);
  } else {
    hipLaunchKernelGGL(rb_scan2_kernel, dim3(gy), dim3(1024), 0, s, counts2, tab, gx, gy, ranges);
    hipLaunchKernelGGL(rb_scatter2_kernel<false>, dim3(nb2 + nb_apply), dim3(RB_THREADS), 0, s, ent, capacity, tab, counts2, list,
                       capacity, nb2, pg, gx, gy, ranges);
  }
  return {rb_launch_status(ctx), fused2};
}
