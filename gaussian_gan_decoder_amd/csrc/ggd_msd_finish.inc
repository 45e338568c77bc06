// ggd_msd_finish.inc -- the per-bucket half of the two-launch depth sort (GGD_MSD_*, ggd_common.h), included inside the anonymous
// namespace of ggd_binning.hip (sort_msd_finish_kernel).  Needs ggd_scan.inc (wave_inclusive_scan); MSD_TILE = the 4096 keys of a tile of launch 1 (ggd_binning_layout.h).  (Kept as an include since
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
                                                int ntiles, uint32_t nb, int kshift, uint32_t* xk_g, uint32_t* xv_g) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
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
    for (int z = tid; z < MSDF_WAVES * 128; z += MSDF_THREADS) reinterpret_cast<uint32_t*>(&L.cnt[0][0])[z] = 0u;
    __syncthreads();
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
        if (GLOBAL_X) { xk_g[p] = key[r]; xv_g[p] = val[r]; }
        else { L.kv[p] = key[r]; L.kv[MSD_XCAP + p] = val[r]; }
      }
    }
    __syncthreads();
  }
}
