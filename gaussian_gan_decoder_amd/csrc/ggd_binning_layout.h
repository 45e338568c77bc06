// ggd_binning_layout.h -- every buffer layout of the forward front end (depth sort, folded front end, row binning), once.
//
// Host arithmetic only: sizes, offsets and the constants they are made of.  ggd_binning.hip and ggd_rowbin.hip take their
// pointers from here, ggd_capi.hip / ggd_knn.hip / ggd_triplane.hip their sizes and the device words they read behind the
// sort; no other file adds an offset to a control block or to the row binning's scratch.  Includes <stdint.h> and <stddef.h>
// only, so that tests/host/binning_layout.cpp can compile it with the system C++ compiler (as ggd_spec.h).
#pragma once

#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define GGD_HOST_DEVICE __host__ __device__
#else
#define GGD_HOST_DEVICE
#endif

static inline size_t ggd_align(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------- onesweep sort ---
constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 16;                      // keys per lane
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;    // 4096 pairs per tile
constexpr int RS_BINS = 256;
constexpr int RS_MAX_PASSES = 8;
constexpr int RS32_ITEMS = 16;                   // tile size of the 32-bit (depth) sort (4 was slower: longer look-back)
constexpr int RS32_TILE = RS_THREADS * RS32_ITEMS;
constexpr int RS_HWORDS = RS_MAX_PASSES * RS_BINS;
constexpr int RS_RESIDENT = 1024;   // tiles (256-thread workgroups, 5 KB LDS) that are certainly resident together on 256 CUs

// Two-level look-back (ggd_lookback.inc): tiles per group = 2^shift, the smallest shift >= 2 with 4^shift >= n -- the power of
// two nearest to sqrt(n) from above.  THE definition: the hosts size the group words with it, the kernels index them with it
// (T = the caller's count type, so that a kernel keeps its own integer width).
template <typename T>
GGD_HOST_DEVICE inline int ggd_group_shift(T n) { int g = 2; while (((T)1 << (2 * g)) < n) ++g; return g; }

// status words per pass: tile words, then group words.  A pass picks its group size from the number of tiles that hold elements
// (a device-side count in the compacting sort): g <= ggd_group_shift(ntiles) with up to 2^g groups in use -- more than
// ntiles >> ggd_group_shift(ntiles) when the count falls just below a power of four (257 launched tiles, 256 live ones: 16 groups
// against 9 rows; the overflow landed in the next pass's tile words).  2^shift + 1 rows cover every choice.
static inline int64_t rs_status_words(int64_t ntiles) {
  return (ntiles + ((int64_t)1 << ggd_group_shift(ntiles)) + 1) * RS_BINS;
}
static inline int64_t ggd_tiles(int64_t n, int tile) { const int64_t t = (n + tile - 1) / tile; return t > 0 ? t : 1; }

// control block in front of the status words: [ghist: MAX_PASSES * 256][tickets: MAX_PASSES][n_valid][flat][pad to 64 words]
static inline size_t ggd_sort_ctrl_bytes() { return ggd_align((size_t)(RS_HWORDS + 64) * sizeof(uint32_t)); }
static inline size_t ggd_sort_ctrl_words() { return ggd_sort_ctrl_bytes() / sizeof(uint32_t); }   // (what clean_ctl must hold)
// tmp of ggd_launch_sort (64-bit keys, up to 8 passes) / ggd_launch_sort32_iota (4 passes): [control block | status words]
static inline size_t ggd_sort_tmp_bytes(int64_t n) {
  return ggd_sort_ctrl_bytes() + ggd_align((size_t)RS_MAX_PASSES * (size_t)rs_status_words(ggd_tiles(n, RS_TILE)) * sizeof(uint32_t));
}
static inline size_t ggd_sort32_tmp_bytes(int64_t n) {
  return ggd_sort_ctrl_bytes() + ggd_align((size_t)4 * (size_t)rs_status_words(ggd_tiles(n, RS32_TILE)) * sizeof(uint32_t));
}
// status words of `passes` passes over `ntiles` tiles; with the control block in front: what a sort that owns its tmp clears
static inline size_t ggd_sort_status_words(int passes, int64_t ntiles) { return (size_t)passes * (size_t)rs_status_words(ntiles); }
static inline size_t ggd_sort_clear_bytes(int passes, int64_t ntiles) {
  return ggd_sort_ctrl_bytes() + ggd_sort_status_words(passes, ntiles) * sizeof(uint32_t);
}

// -------------------------------------------------------------------------- two-launch depth sort, folded front end ---
constexpr int GGD_MSD_BINS = 1024, GGD_MSD_CAP = 12288, GGD_MSD_MAX_TILES = 2048;
constexpr int MSD_ITEMS = 16;                       // launch 1: 4096 keys per tile, as the onesweep passes
constexpr int MSD_TILE = 256 * MSD_ITEMS;
static inline size_t ggd_sort32_msd_table_bytes(int64_t n) {   // table[tile][bucket]
  return ggd_align((size_t)ggd_tiles(n, MSD_TILE) * GGD_MSD_BINS * sizeof(uint32_t));
}

// Fold block (words; described at ggd_fold, ggd_common.h):
//   [REPS replicas of REP_STRIDE histogram words | 8 tickets | n_valid | flat | pad | OUTSIDE (word 16 behind the histograms, a
//    line of its own) | pad to 64 | ROWTOT: REPS x 64 entries per tile row | status words of the 4 passes | level-1 status words |
//    ROWINST: REPS x 64 instances per tile row]
constexpr int GGD_FOLD_REPS = 16;   // (32 / 16 / 8 replicas: 4114 / 4140 / 4150 frames per second at 1 M / 1024^2; 3907 workgroups over 8 would
                                    // keep one address busy 80 % of the kernel's time, 16 leaves a margin)
constexpr int GGD_FOLD_REP_STRIDE = GGD_MSD_BINS + 256;   // ordinary frames: the four byte histograms [p * 256 + digit] in the first
                                               // 1024 words; two-launch sort: [1024 buckets of the key window | 256 bins of the top byte]
constexpr int GGD_FOLD_OUTSIDE = GGD_FOLD_REPS * GGD_FOLD_REP_STRIDE + 16;   // kept keys outside the two-launch sort's window
constexpr int GGD_FOLD_ROWTOT = GGD_FOLD_REPS * GGD_FOLD_REP_STRIDE + 64;   // REPS x 64 words: entries per tile ROW (grids of <= 64
                                                                           // rows), for the row binning's first level
constexpr int GGD_FOLD_HEAD = GGD_FOLD_ROWTOT + GGD_FOLD_REPS * 64;        // words in front of the status words
static inline size_t ggd_fold_l1_offset(int64_t P) {   // first word of the level-1 status words
  return (size_t)GGD_FOLD_HEAD + (size_t)4 * (size_t)rs_status_words(ggd_tiles(P, RS32_TILE));
}
static inline size_t ggd_fold_ctl_words(int64_t P) {   // + level-1 binning: one 64-word row per 1024-Gaussian chunk and per group of chunks
  const int64_t chunks = (P + 1023) / 1024;
  return ggd_fold_l1_offset(P) + (size_t)(chunks + ((int64_t)1 << ggd_group_shift(chunks > 0 ? chunks : 1)) + 2) * 64;
}
// REPS x 64 words behind the level-1 status words: INSTANCES per tile row (the row's entries weighted by their width in tiles) --
// the only cross-row quantity of the row binning's second level, which then needs no scan launch (rb_scatter2_kernel<true>).
// Appended, so that every offset above keeps its value; ggd_fold_block_words is what a fold block holds in all.
static inline size_t ggd_fold_rowinst_offset(int64_t P) { return ggd_fold_ctl_words(P); }
static inline size_t ggd_fold_block_words(int64_t P) { return ggd_fold_rowinst_offset(P) + (size_t)GGD_FOLD_REPS * 64; }
static inline uint32_t* ggd_fold_rowtot(uint32_t* fold_ctl) { return fold_ctl + GGD_FOLD_ROWTOT; }
static inline uint32_t* ggd_fold_rowinst(uint32_t* fold_ctl, int64_t P) { return fold_ctl + ggd_fold_rowinst_offset(P); }
static inline uint32_t* ggd_fold_l1_status(uint32_t* fold_ctl, int64_t P) { return fold_ctl + ggd_fold_l1_offset(P); }

// The sort's control block in its three forms.  n_valid: kept keys (the element count of every pass after the first and of the
// consumers), flat: "the last pass was the identity, the result is in (keys_b, vals_b)" -- device words both.
struct ggd_sort_ctl {
  uint32_t* ghist = nullptr;     // [reps] replicas of the passes' histograms
  uint32_t* tickets = nullptr;   // [RS_MAX_PASSES]
  uint32_t* n_valid = nullptr;
  uint32_t* flat = nullptr;
  uint32_t* status = nullptr;    // [passes][rs_status_words(ntiles)]
  int reps = 1;

  // head of tmp (the sort clears it itself)
  static ggd_sort_ctl in_tmp(void* tmp) {
    return make(static_cast<uint32_t*>(tmp), RS_HWORDS, tmp_status(tmp), 1);
  }
  // a block an earlier kernel of the frame has cleared; the status words stay in tmp (cleared by the histogram kernel)
  static ggd_sort_ctl in_clean(uint32_t* clean_ctl, void* tmp) { return make(clean_ctl, RS_HWORDS, tmp_status(tmp), 1); }
  // a fold block: status words included, cleared by the previous frame's preprocess, histograms filled by this frame's
  static ggd_sort_ctl in_fold(uint32_t* fold_ctl) {
    return make(fold_ctl, GGD_FOLD_REPS * GGD_FOLD_REP_STRIDE, fold_ctl + GGD_FOLD_HEAD, GGD_FOLD_REPS);
  }
  // ... whichever the caller has: a fold block wins, then a clean block
  static ggd_sort_ctl select(void* tmp, uint32_t* clean_ctl, uint32_t* fold_ctl) {
    return fold_ctl ? in_fold(fold_ctl) : (clean_ctl ? in_clean(clean_ctl, tmp) : in_tmp(tmp));
  }

  uint32_t* pass_hist(int p) const { return ghist + p * RS_BINS; }
  uint32_t* pass_ticket(int p) const { return tickets + p; }
  uint32_t* pass_status(int p, int64_t ntiles) const { return status + ggd_sort_status_words(p, ntiles); }

 private:
  static uint32_t* tmp_status(void* tmp) { return reinterpret_cast<uint32_t*>(static_cast<char*>(tmp) + ggd_sort_ctrl_bytes()); }
  static ggd_sort_ctl make(uint32_t* head, int hist_words, uint32_t* status, int reps) {
    ggd_sort_ctl c;
    c.ghist = head; c.tickets = head + hist_words; c.n_valid = c.tickets + RS_MAX_PASSES; c.flat = c.n_valid + 1;
    c.status = status; c.reps = reps;
    return c;
  }
};

// ------------------------------------------------------------------------------------------------ row binning ---
constexpr int RB_THREADS = 256;
constexpr int RB_IPL = 4;                          // items per lane (2 and 8 measured slower)
constexpr int RB_CHUNK = RB_THREADS * RB_IPL;      // 1024 items per workgroup
// tables, grids up to 64 x 64 (uint32): [0..64] row starts (65 entries, [64] = total entries), [65..129] first level-2 block of
// each row (+ total), [130 .. 130 + 64*64) start of every (row, column) tile list, [ROWINST + r] instances of row r,
// [FLAG + r] != 0 once it is published (level-2 scan, one workgroup per row)
constexpr int RB_TAB_ROWSTART = 0, RB_TAB_ROWBLK = 65, RB_TAB_TILESTART = 130, RB_TAB_ROWINST = 130 + 64 * 64,
              RB_TAB_FLAG = RB_TAB_ROWINST + 64, RB_TAB_WORDS = RB_TAB_FLAG + 64;
// tables, grids up to 255 x 255 (ggd_rowbin_wide.inc), strides fixed at RBW_BINS whatever the grid:
//   [ROWSTART .. +256]  start of every tile row's entry list (+ total)      [ROWBLK .. +256]  first level-2 block of each row (+ total)
//   [ROWINST + r] instances of row r, [FLAG + r] != 0 once published        [TILESTART + r * 256 + c] start of tile (r, c)'s list
constexpr int RBW_NG = 4;                 // groups of 64 bins
constexpr int RBW_BINS = 64 * RBW_NG;     // 256 (bins 0 .. 254 are usable: a rect's exclusive upper bound must fit 8 bits)
constexpr int RBW_TAB_ROWSTART = 0, RBW_TAB_ROWBLK = RBW_BINS + 1, RBW_TAB_ROWINST = 2 * (RBW_BINS + 1),
              RBW_TAB_FLAG = RBW_TAB_ROWINST + RBW_BINS, RBW_TAB_TILESTART = RBW_TAB_FLAG + RBW_BINS,
              RBW_TAB_WORDS = RBW_TAB_TILESTART + RBW_BINS * RBW_BINS;

// The `packed` record, one per depth rank: {id, x0 | x1 << 8 | y0 << 16 | y1 << 24} -- the tile rect [x0, x1) x [y0, y1) in bytes
// (grids up to 255 x 255), all zero for an empty rect.  Written by rb_count1_kernel / rbw_count1_kernel and by the depth sort's
// finish launch (msd_count_rows, ggd_msd_finish.inc); read by the level-1 scatters and by rb_level1_counted_kernel.
GGD_HOST_DEVICE inline uint32_t rb_pack_rect(uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {
  return x0 | (x1 << 8) | (y0 << 16) | (y1 << 24);
}
GGD_HOST_DEVICE inline uint32_t rb_packed_cols(uint32_t w) { return w & 0xffffu; }       // x0 | x1 << 8: the payload of a row entry
GGD_HOST_DEVICE inline uint32_t rb_packed_rows(uint32_t w) { return w >> 16; }           // y0 | y1 << 8: the interval of rows
GGD_HOST_DEVICE inline uint32_t rb_packed_y0(uint32_t w) { return (w >> 16) & 0xffu; }
GGD_HOST_DEVICE inline uint32_t rb_packed_y1(uint32_t w) { return w >> 24; }

static inline bool rb_is_wide(int W, int H) { return (W + 15) / 16 > 64 || (H + 15) / 16 > 64; }
static inline int rb_blocks1(int P) { return (P + RB_CHUNK - 1) / RB_CHUNK; }                      // level-1 workgroups
// The scan-in-scatter form of level 2 (rb_scatter2_kernel<true>) has every workgroup of a tile row read the count rows of all of
// the row's blocks: 256 bytes x (blocks of the row)^2 per row, a device-side figure.  The host only knows the launched blocks (one
// per 1024 instances of CAPACITY; the live ones cover the row entries: 1200 of 5857 on the 1 M cube, 3200 of 16449 on the shell),
// so the form is taken for capacities up to 2^24 instances -- what the 1 M shell needs (2^24 + 1) and no more.  Worst case
// admitted: 2^24 one-tile-wide entries in ONE tile row, 16384 blocks, 16384^2 rows of 256 bytes = 69 GB of cache reads (reasoned, not
// timed: DESIGN.md 6o); spread over the 64 rows, 1/64 of that.  Larger frames keep rb_scan2_kernel.
constexpr uint32_t RB_SCAN_IN_SCATTER_MAX_BLOCKS = (1u << 24) / RB_CHUNK + 128;
static inline uint32_t rb_blocks2(uint32_t cap, bool wide) {                                       // level-2 workgroups: a ragged
  return (cap + RB_CHUNK - 1) / RB_CHUNK + (wide ? (uint32_t)RBW_BINS : 64u);                      // last chunk per tile row
}

// The row binning's scratch (byte offsets into tmp), both widths: the depth-ordered rects, level 1's per-chunk counts (nby bins
// a chunk), the tables, the row entries, level 2's per-chunk counts (nbx bins a chunk).  nby / nbx: 64 bins per group of rows /
// columns the grid needs (64 on the narrow path).
// Counted level 1 (rb_level1_counted_kernel; frames of the two-launch sort on the narrow path): two row tables BEHIND `total`, so
// that every offset above and `total` itself keep their values -- `total` is what the other forms need, `total_counted` what a
// caller that may take the counted form reserves.
//   bucket_rows[GGD_MSD_BINS][64]      row entries per tile row of every bucket of the two-launch sort
//   boundary_rows[rb_blocks1(P)][64]   ... of the elements of the bucket that holds rank 1024 k in front of that rank
// both written by sort_msd_finish_kernel with plain stores, read by the launch behind it.
struct ggd_rowbin_tmp {
  size_t packed, counts1, tab, ent, counts2, total;
  size_t bucket_rows, boundary_rows, total_counted;
};
static inline ggd_rowbin_tmp ggd_rowbin_layout(int P, uint32_t capacity, int W, int H) {
  const bool wide = rb_is_wide(W, H);
  const int nby = 64 * (((H + 15) / 16 + 63) / 64), nbx = 64 * (((W + 15) / 16 + 63) / 64);
  ggd_rowbin_tmp t;
  t.packed = 0;
  t.counts1 = t.packed + ggd_align((size_t)P * 8);
  t.tab = t.counts1 + ggd_align((size_t)rb_blocks1(P) * (wide ? nby : 64) * 4);
  t.ent = t.tab + ggd_align((size_t)(wide ? RBW_TAB_WORDS : RB_TAB_WORDS) * 4);
  t.counts2 = t.ent + ggd_align((size_t)capacity * 8);
  t.total = t.counts2 + ggd_align((size_t)rb_blocks2(capacity, wide) * (wide ? nbx : 64) * 4);
  t.bucket_rows = t.total;
  t.boundary_rows = t.bucket_rows + ggd_align((size_t)GGD_MSD_BINS * 64 * 4);
  t.total_counted = t.boundary_rows + ggd_align((size_t)rb_blocks1(P) * 64 * 4);
  return t;
}
