// ggd_msd_finish.inc -- the per-bucket half of the two-launch depth sort (GGD_MSD_*, ggd_common.h), included inside the anonymous
// namespace of ggd_binning.hip (sort_msd_finish_kernel).  Needs ggd_lanes.h (wave_inclusive_scan); MSD_TILE = the 4096 keys of a tile of launch 1 (ggd_binning_layout.h).  (Kept as an include since
// round 5's experiment of running level 1 of the binning on the sorted bucket inside the same workgroup -- one launch and one
// gather chain less, but 48.8 us against 16.5 + 23.0 for the two kernels: profiles/REJECTED.md.)
//
// Workgroup b owns bucket b (keys whose offset inside the frame's key window, key - lo, has the high part b = offset >> shift;
// launch 1 stored the offsets).  Its elements sit in up to `ntiles` pieces, one per tile of launch 1, each already in index
// order; taken in tile order they are in index order throughout, so stable counting passes over the offset's bits 0..7 and
// 8..shift-1 (shift <= 16; the second pass is skipped for shift <= 8) leave them in the order of a stable sort of the whole
// key.  1024 threads, <= 12 elements each, all in registers between the passes.
constexpr int MSDF_THREADS = 1024, MSDF_ITEMS = GGD_MSD_CAP / MSDF_THREADS, MSDF_WAVES = MSDF_THREADS / 64;
static_assert(MSDF_ITEMS * MSDF_THREADS == GGD_MSD_CAP, "bucket capacity must be a multiple of the workgroup size");

__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t* total, uint32_t* lds16) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t inc = wave_inclusive_scan(v);
  if (lane == 63) lds16[wv] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MSDF_WAVES; ++w) {
    const uint32_t s = lds16[w];
    if (w < wv) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// Buckets of up to MSD_XCAP keys exchange their elements between the two passes through LDS; larger ones (up to GGD_MSD_CAP)
// through their own slice of the output arrays (L2-resident; pass 2 then writes the final order in place -- 1.6 x slower per
// key than LDS, for the rare dense bucket).  With the whole capacity in LDS (96 KB + 32 KB of tables, 70 VGPRs) a CU held ONE
// workgroup: the headline scene's 257 non-empty buckets ran as 256 + 1.  Now 64 000 B of pairs + 16-bit counts + ONE packed word
// per piece = 80 448 B and <= 64 VGPRs: two workgroups per CU, and the head-like scene's 7 k-key buckets still sort in LDS.
// (One word per element in LDS -- 14 key bits + the position in the gathered bucket, key and value fetched again at the end --
// fits 12288 elements in 48 KB, but the second binary search + dependent gather cost more than they saved: 16.0 / 34 us.)
constexpr int MSD_XCAP = 8000;
constexpr int MSDX_ITEMS = (MSD_XCAP + MSDF_THREADS - 1) / MSDF_THREADS;
struct msd_lds {
  uint32_t kv[2 * MSD_XCAP];             // keys [0, XCAP), values [XCAP, 2 XCAP)
  uint16_t cnt[MSDF_WAVES][256];
  uint32_t pp[GGD_MSD_MAX_TILES];        // piece of tile t: nb <= CAP: (first position inside the bucket) << 12 | first slot inside
                                         // the tile; oversized bucket: the first position alone (the slot is read from the table)
  uint32_t part[MSDF_WAVES];
};
static_assert(2 * sizeof(msd_lds) <= 160 * 1024, "two finish workgroups per CU");
static_assert(GGD_MSD_MAX_SHIFT <= 16, "two 8-bit passes order the bits below the bucket digit");
static_assert(GGD_MSD_CAP < (1 << 20) && MSD_TILE <= (1 << 12), "packed piece word");

// position p of bucket b -> index into launch 1's output (the largest tile whose piece starts at or before p: not empty, the
// next one starts behind p)
__device__ __forceinline__ size_t msd_piece_src(const msd_lds& L, int ntiles, uint32_t p) {
  int lo = 0;
#pragma unroll
  for (int step = GGD_MSD_MAX_TILES / 2; step >= 1; step >>= 1) {
    const int probe = lo + step;
    if (probe < ntiles && (L.pp[probe] >> 12) <= p) lo = probe;
  }
  const uint32_t e = L.pp[lo];
  return (size_t)lo * MSD_TILE + (e & 0xfffu) + (p - (e >> 12));
}
// the same for an oversized bucket (L.pp = plain positions; the slot comes from the table)
__device__ __forceinline__ size_t msd_piece_src_big(const msd_lds& L, const uint32_t* __restrict__ table, uint32_t b, int ntiles, uint32_t p) {
  int lo = 0;
#pragma unroll
  for (int step = GGD_MSD_MAX_TILES / 2; step >= 1; step >>= 1) {
    const int probe = lo + step;
    if (probe < ntiles && L.pp[probe] <= p) lo = probe;
  }
  return (size_t)lo * MSD_TILE + (table[(size_t)lo * GGD_MSD_BINS + b] >> 16) + (p - L.pp[lo]);
}

// Step 1 (every thread of the workgroup): the bucket's pieces -- L.pp filled, a barrier behind them.  e0 = the table entry of
// tile threadIdx.x, requested by the caller together with its other loads.
__device__ __forceinline__ void msd_bucket_pieces(msd_lds& L, const uint32_t* __restrict__ table, int ntiles, uint32_t b, uint32_t e0,
                                                  bool oversized) {
  const int tid = threadIdx.x;
  uint32_t carry = 0;
  for (int t0 = 0; t0 < ntiles; t0 += MSDF_THREADS) {
    const int t = t0 + tid;
    const uint32_t e = t0 == 0 ? e0 : (t < ntiles ? table[(size_t)t * GGD_MSD_BINS + b] : 0u);
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan_1024(e & 0xffffu, &tot, L.part);
    // (an EMPTY piece behind a tile's last key starts at slot 4096 when all 4096 keys of the tile were kept: 13 bits -- masked,
    // its slot is never used)
    if (t < ntiles) L.pp[t] = oversized ? carry + ex : ((carry + ex) << 12) | ((e >> 16) & 0xfffu);
    carry += tot;
  }
  __syncthreads();
}

// The rows for the counted level 1 of the row binning (ggd_l1_counted, ggd_common.h).  Once an element's place p in the sorted bucket
// is known it has depth rank base + p; with its rect -- the gather level 1 used to do through `order` -- the workgroup
//   * stores {id, rect in bytes} to packed[base + p],
//   * counts the tile rows the element covers in an LDS difference array, one per 1024-rank chunk the bucket (or one window of
//     <= GGD_MSD_CAP elements of an oversized one) overlaps: <= MSD_ROW_SEGS of 65 words, by the rule of rb_level1_kernel (an
//     empty rect covers nothing; rows are counted as wave_cols counts them).
// Wave 0 (lane = row; `run` = the rows of the bucket's elements in front of the window) then walks the chunks: in front of chunk
// k0 + s it has the rows of the bucket's elements below rank 1024 (k0 + s) -- boundary_rows of that chunk, when the boundary lies
// inside the window (s > 0, or the window starts on it: a bucket that starts on a boundary writes its zero row) -- and behind the
// bucket's last window the bucket's total.  Exactly one non-empty bucket holds a given rank below the kept count, so every row of
// either table has one writer: plain stores, read by the next launch.
// Two forms.  LDS exchange (the usual bucket): inside the LAST counting pass of msd_bucket_sort -- the rects are requested when
// the pass has its values and are looked at when it scatters, a whole pass later; the scatter leaves the rect's bytes where the
// sorted keys went (nobody reads those), so `packed` leaves with the values as coalesced stores; the difference arrays live in
// L.pp, which is dead behind the gather.  Global exchange and oversized buckets (rare): msd_bucket_rows, behind the sort, from the
// workgroup's own slice of vals_out; the difference arrays live in L.cnt.
// Bounds: p < nb and base + nb <= the histogram's total <= P (rank < R.n states it again where `packed` is stored); the chunk index
// is < MSD_ROW_SEGS because a window holds <= GGD_MSD_CAP elements (and is clamped); rows are clamped to 64, the last word of a
// difference array; a rect is read at min(id, R.n - 1); boundary rows are written for k < R.chunks only; b < GGD_MSD_BINS is the
// launch's grid.
constexpr int MSD_ROW_SEGS = GGD_MSD_CAP / 1024 + 1;
static_assert(MSD_ROW_SEGS * 65 * sizeof(int) <= sizeof(msd_lds::cnt) && MSD_ROW_SEGS * 65 * sizeof(int) <= sizeof(msd_lds::pp),
              "the row difference arrays reuse the digit counts / the piece table");
struct msd_rows {
  const uint2* rect; uint2* packed; uint32_t* bucket_rows; uint32_t* boundary_rows;
  uint32_t chunks, n;
};

// the element of depth rank `rank` with rect rc: counted in diff (whose first array is chunk k0's); returns the rect in bytes
// (the `packed` record's second word, rb_pack_rect).  Unlike rb_count1_kernel this writer cannot rely on the grid for its bounds --
// the rows index LDS here -- so rows are clamped to 64 and the columns masked to their byte before they are packed.
__device__ __forceinline__ uint32_t msd_count_rows(int* diff, uint32_t k0, uint32_t rank, uint2 rc) {
  uint32_t x0 = rc.x & 0xffffu, x1 = rc.x >> 16, y0 = min(rc.y & 0xffffu, 64u), y1 = min(rc.y >> 16, 64u);
  const bool any = (int)(x1 - x0) * (int)(y1 - y0) > 0 && y1 > y0;
  if (!any) return 0u;
  const uint32_t s = min((rank >> 10) - k0, (uint32_t)(MSD_ROW_SEGS - 1));
  atomicAdd(&diff[s * 65u + y0], 1);
  atomicAdd(&diff[s * 65u + y1], -1);
  return rb_pack_rect(x0 & 0xffu, x1 & 0xffu, y0, y1);
}

// wave 0 (tid = row), a barrier behind the counting: the window [first, end) of depth ranks, `last`: the bucket ends with it
__device__ __forceinline__ void msd_publish_rows(const int* diff, const msd_rows& R, uint32_t b, uint32_t first, uint32_t end, bool last,
                                                 uint32_t& run) {
  const int tid = threadIdx.x;
  const uint32_t k0 = first >> 10;
  const uint32_t nseg = min(((end - 1u) >> 10) - k0 + 1u, (uint32_t)MSD_ROW_SEGS);
  for (uint32_t s = 0; s < nseg; ++s) {
    const uint32_t k = k0 + s;
    if ((s > 0u || (first & 1023u) == 0u) && k < R.chunks) R.boundary_rows[(size_t)k * 64 + tid] = run;
    run += (uint32_t)wave_inclusive_scan(diff[s * 65u + tid]);
  }
  if (last) R.bucket_rows[(size_t)b * 64 + tid] = run;
}

// the form behind the sort: elements [p0, p0 + GGD_MSD_CAP) of the bucket, whose order is in vals_g[0, nb) (a barrier behind it)
__device__ __forceinline__ void msd_bucket_rows(msd_lds& L, const msd_rows& R, uint32_t b, uint32_t base, uint32_t nb, uint32_t p0,
                                                uint32_t& run, const uint32_t* vals_g) {
  const int tid = threadIdx.x;
  int* diff = reinterpret_cast<int*>(&L.cnt[0][0]);   // [MSD_ROW_SEGS][65]
  const uint32_t p1 = min(nb, p0 + (uint32_t)GGD_MSD_CAP);
  const uint32_t k0 = (base + p0) >> 10;
  for (uint32_t z = tid; z < (uint32_t)(MSD_ROW_SEGS * 65); z += MSDF_THREADS) diff[z] = 0;
  __syncthreads();
  // four elements a thread at a time, their gathers requested together (all twelve at once cost the kernel its 64-register budget)
  constexpr int RB = 4;
#pragma unroll 1
  for (uint32_t q0 = p0; q0 < p1; q0 += (uint32_t)(RB * MSDF_THREADS)) {
    uint32_t id[RB];
    uint2 rc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const uint32_t p = q0 + (uint32_t)(r * MSDF_THREADS + tid);
      id[r] = 0u; rc[r] = make_uint2(0u, 0u);
      if (p < p1) {
        id[r] = vals_g[p];
        rc[r] = R.rect[min(id[r], R.n - 1u)];
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const uint32_t p = q0 + (uint32_t)(r * MSDF_THREADS + tid);
      if (p < p1 && base + p < R.n) R.packed[base + p] = make_uint2(id[r], msd_count_rows(diff, k0, base + p, rc[r]));
    }
  }
  __syncthreads();
  if (tid < 64) msd_publish_rows(diff, R, b, base + p0, base + p1, p1 == nb, run);
}

// Step 2 (nb <= GGD_MSD_CAP): gather + two stable counting passes over the offsets' bits 0..7 and 8..shift-1.  LDS exchange (GLOBAL_X =
// false, nb <= MSD_XCAP, ITEMS = MSDX_ITEMS): on return the sorted keys are in L.kv[0, nb), their values in L.kv[XCAP, XCAP +
// nb), a barrier behind them.  Global exchange (GLOBAL_X = true): xk / xv = the bucket's slice of the output arrays; on return
// they hold the sorted bucket.  Pass 2 reads its elements from the exchange arrays, and three barriers separate those reads from
// its scatter into the same arrays.
// Element p of the bucket belongs to (wave, round, lane) = (p / (64 rounds), (p / 64) % rounds, p % 64), rounds = ceil(nb / 1024):
// every wave owns a contiguous run of the bucket (stable ranking: earlier waves, then earlier rounds, then lower lanes) and all
// sixteen waves share the work of a small bucket (a fixed 12 rounds per wave left a typical 1400-key bucket to two waves: 86
// instead of 16 us).
template <bool GLOBAL_X, int ITEMS>
__device__ __forceinline__ void msd_bucket_sort(msd_lds& L, const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                int ntiles, uint32_t nb, int kshift, uint32_t* xk_g, uint32_t* xv_g,
                                                const msd_rows& R, uint32_t base) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
  // LDS exchange with a counted level 1 behind: the last pass also fetches the rects and counts the rows (see above); on return
  // L.kv[0, nb) holds the rects' bytes instead of the sorted keys and diff the counts, a barrier behind both
  const bool rows_here = !GLOBAL_X && R.rect != nullptr;
  int* diff = reinterpret_cast<int*>(&L.pp[0]);   // [MSD_ROW_SEGS][65]
  constexpr int EARLY = GLOBAL_X ? 1 : 4;         // rounds whose rects are requested a pass ahead (buckets up to 4096 keys: all but the
  uint2 rc[EARLY];                                // dense ones; every round's cost the kernel its 64-register budget)
  const int rounds = (int)((nb + MSDF_THREADS - 1) / MSDF_THREADS);
  const uint32_t pbase = (uint32_t)wv * (64u * (uint32_t)rounds) + (uint32_t)lane;
#pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    if (r >= rounds) break;
    const uint32_t p = pbase + r * 64;
    key[r] = 0u; val[r] = 0u;
    if (p < nb) {
      const size_t src = msd_piece_src(L, ntiles, p);
      key[r] = keys_in[src];
      val[r] = vals_in[src];
    }
  }
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int shift = 8 * pass;
    const int nbits = pass == 0 ? min(8, kshift) : kshift - 8;   // (the bits from kshift up are the same for every key of a bucket)
    if (pass == 1 && nbits <= 0) break;                    // (wave-uniform: a kernel argument)
    if (pass == 1) {
#pragma unroll
      for (int r = 0; r < ITEMS; ++r) {
        if (r >= rounds) break;
        const uint32_t p = pbase + r * 64;
        if (p < nb) {
          if (GLOBAL_X) { key[r] = xk_g[p]; val[r] = xv_g[p]; }
          else { key[r] = L.kv[p]; val[r] = L.kv[MSD_XCAP + p]; }
        }
      }
    }
    const bool count_rows = rows_here && (pass == 1 || kshift <= 8);   // (this is the last pass)
    if constexpr (!GLOBAL_X) {
      if (count_rows) {
#pragma unroll
        for (int r = 0; r < EARLY; ++r) {   // requested here, looked at in the scatter below
          if (r >= rounds) break;
          rc[r] = make_uint2(0u, 0u);
          if (pbase + r * 64 < nb) rc[r] = R.rect[min(val[r], R.n - 1u)];
        }
      }
    }
    for (int z = tid; z < MSDF_WAVES * 128; z += MSDF_THREADS) reinterpret_cast<uint32_t*>(&L.cnt[0][0])[z] = 0u;
    __syncthreads();
    if (count_rows) {   // (behind the barrier: pass 0's gather has read L.pp for the last time)
      for (int z = tid; z < MSD_ROW_SEGS * 65; z += MSDF_THREADS) diff[z] = 0;
    }
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
      if (r >= rounds) break;
      const bool ok = pbase + r * 64 < nb;
      const uint32_t d = (key[r] >> shift) & ((1u << nbits) - 1u);
      uint64_t peers = __ballot(ok);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        if (bit >= nbits) break;
        const uint64_t m = __ballot((d >> bit) & 1u);
        peers &= ((d >> bit) & 1u) ? m : ~m;
      }
      const uint32_t before = L.cnt[wv][d];
      const uint32_t below = (uint32_t)__popcll(peers & lt_mask);
      rank[r] = before + below;
      __builtin_amdgcn_wave_barrier();
      if (ok && below == 0) L.cnt[wv][d] = (uint16_t)(before + (uint32_t)__popcll(peers));
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
      // thread d < 256 owns digit d: its first slot = digits below + the same digit in earlier waves (the sixteen per-wave
      // counts are read twice rather than held: sixteen live registers per thread spilled)
      uint32_t local = 0;
      if (tid < 256) {
#pragma unroll
        for (int w = 0; w < MSDF_WAVES; ++w) local += L.cnt[w][tid];
      }
      uint32_t tot;
      uint32_t run = block_exclusive_scan_1024(tid < 256 ? local : 0u, &tot, L.part);
      if (tid < 256) {
#pragma unroll
        for (int w = 0; w < MSDF_WAVES; ++w) { const uint32_t c = L.cnt[w][tid]; L.cnt[w][tid] = (uint16_t)run; run += c; }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
      if (r >= rounds) break;
      if (pbase + r * 64 < nb) {
        const uint32_t d = (key[r] >> shift) & ((1u << nbits) - 1u);
        const uint32_t p = (uint32_t)L.cnt[wv][d] + rank[r];
        if constexpr (GLOBAL_X) { xk_g[p] = key[r]; xv_g[p] = val[r]; }
        else {
          L.kv[p] = !count_rows ? key[r]
                               : msd_count_rows(diff, base >> 10, base + p, r < EARLY ? rc[r < EARLY ? r : 0] : R.rect[min(val[r], R.n - 1u)]);
          L.kv[MSD_XCAP + p] = val[r];
        }
      }
    }
    __syncthreads();
  }
}
