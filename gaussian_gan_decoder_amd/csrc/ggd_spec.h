// ggd_spec.h -- the cross-frame speculation policy of the single-call forward, as plain host code (no HIP: tests/host/ runs it).
//
// The depth sort has two short forms that are only valid for some frames; the host picks one BEFORE it knows the frame, from what
// the frames before it reported, and the frame's own front end reports (with num_rendered) whether the pick held:
//   three passes      the fourth onesweep pass is not launched.  Valid when the kept keys' top byte is constant ("flat").
//                     Picked after GGD_FLAT_STREAK flat folded frames in a row; one non-flat folded frame zeroes the streak.
//   two launches      one partition over a key window [lo, lo + buckets << shift) + an in-LDS finish (ggd_common.h).  Valid when no
//                     kept key lies outside the window and no bucket is oversized.  The window is the union of the kept-key ranges
//                     of the last (up to GGD_MSD_WIN) folded frames + 1/8 margin; picked once GGD_FLAT_STREAK ranges are known and
//                     no pause is running.  It wins over three passes.
// A frame whose pick did not hold is binned and blended again by the exact path (a "rerun").  A key outside the window pauses the
// two-launch form for 2 frames (the frame's range has joined the ring, so the next window contains it); an oversized bucket forgets
// the ring and pauses 8, 16, 32, 64, 64, ... frames while it keeps happening (the ring re-forms from the missing frame's own range);
// one successful two-launch frame ends the doubling.  Pauses and streaks only move on folded frames.
#pragma once

#include <stdint.h>

constexpr int GGD_FLAT_STREAK = 8;
constexpr int GGD_MSD_SHIFT = 14, GGD_MSD_BAN = 64;
constexpr int GGD_MSD_WIN = 32, GGD_MSD_MAX_SHIFT = 16;   // frames whose key ranges form the window; two 8-bit passes finish a bucket
constexpr int GGD_MSD_TARGET = 512;   // buckets the window is spread over: 512 = one resident round of the finish kernel (two workgroups
                                      // per CU); measured at 1 M / 1024^2, sort stage cube / shell: 1024 -> 27.4 / 35.8 us, 512 -> 23.5 / 33.5,
                                      // 256 -> 25.8 / 34.1 (round 5's fixed bits 14..23: 23.2 / 34.5)

struct ggd_spec_plan {     // decided before the preprocess launch: it selects the histograms that launch builds
  bool msd = false;        // the two-launch sort, over buckets = (key - lo) >> shift
  uint32_t lo = 0;
  int shift = GGD_MSD_SHIFT;
};

struct ggd_spec_report {   // what a frame's front end says about it; arrives with num_rendered
  bool folded = false;     // the frame ran the folded front end: the rest is meaningful
  bool flat = false;       // the kept keys' top byte was constant
  bool msd_ok = false;     // the two-launch sort's histograms say it was valid
  uint32_t kmin = 0xffffffffu, kmax = 0u;   // kept-key range (kmin > kmax: nothing was kept)
  uint32_t msd_flags = 0u;                  // bit 2: a kept key outside the window (else a miss is an oversized bucket)
};

struct ggd_spec {
  int flat_streak = 0;
  int msd_ban = 0;               // folded frames to wait before the two-launch sort is planned again
  int msd_oversize_streak = 0;   // consecutive oversized-bucket misses (<= 4)
  uint32_t win_lo[GGD_MSD_WIN], win_hi[GGD_MSD_WIN];   // ring: kept-key min / max of the last folded frames
  int win_n = 0, win_pos = 0;
  int msd_buckets = GGD_MSD_TARGET;   // (GGD_MSD_BUCKETS: timing experiments)
  unsigned long long reruns = 0, msd_frames = 0;   // GGD_STAT_SORT_RERUNS, GGD_STAT_MSD_FRAMES

  // A defined starting point for a caller that switches forms (GGD_OPT_MSD_SORT, GGD_OPT_FOLD); counters and msd_buckets stay.
  void reset() { win_n = 0; win_pos = 0; msd_ban = 0; msd_oversize_streak = 0; flat_streak = 0; }

  // The key window for the next frame: the union of the ring's ranges, a margin of 1/8 of its width (+ 4096) either side, and the
  // smallest shift that spreads it over at most msd_buckets buckets.  False when no range is known or the window is too wide
  // for two 8-bit finishing passes.
  bool fit_window(uint32_t* lo_out, int* shift_out) const {
    const int n = win_n < GGD_MSD_WIN ? win_n : GGD_MSD_WIN;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int i = 0; i < n; ++i) { lo = win_lo[i] < lo ? win_lo[i] : lo; hi = win_hi[i] > hi ? win_hi[i] : hi; }
    if (lo > hi) return false;
    const uint64_t margin = ((uint64_t)(hi - lo) >> 3) + 4096u;
    const uint64_t wlo = (uint64_t)lo > margin ? (uint64_t)lo - margin : 0u;
    uint64_t whi = (uint64_t)hi + margin;
    if (whi > 0xfffffffeull) whi = 0xfffffffeull;
    const uint64_t span = whi - wlo;            // bucket of the largest key = span >> shift, must stay below the bucket count
    int shift = 0;
    while ((span >> shift) >= (uint64_t)msd_buckets) ++shift;
    if (shift > GGD_MSD_MAX_SHIFT) return false;
    *lo_out = (uint32_t)wlo; *shift_out = shift;
    return true;
  }

  // This frame's plan.  fold_opt / msd_opt: GGD_OPT_FOLD / GGD_OPT_MSD_SORT; msd_supported: the two-launch sort takes this P.
  ggd_spec_plan plan(int fold_opt, int msd_opt, bool msd_supported) const {
    ggd_spec_plan p;
    p.msd = msd_opt != 0 && fold_opt == 1 && win_n >= GGD_FLAT_STREAK && msd_ban == 0 && msd_supported && fit_window(&p.lo, &p.shift);
    return p;
  }

  // Launch three sort passes instead of four?  folded: the frame runs the folded front end; speculative: the host has not seen
  // num_rendered yet (a frame that is rendered again is not).
  bool three_passes(const ggd_spec_plan& p, bool folded, bool speculative, int fold_opt) const {
    return !p.msd && folded && speculative && flat_streak >= GGD_FLAT_STREAK && fold_opt == 1;
  }

  // Take in a frame's report; returns whether the frame must be rendered again (counted in `reruns`).  abandoned: the caller gives
  // the frame up (its buffer was too small; it runs it again itself): no rerun.  The order of the steps shows in the counters.
  bool observe(const ggd_spec_plan& p, bool three, const ggd_spec_report& r, bool abandoned = false) {
    if (r.folded) flat_streak = r.flat ? (flat_streak < (1 << 30) ? flat_streak + 1 : flat_streak) : 0;
    if (r.folded && msd_ban > 0) msd_ban -= 1;
    const bool msd_missed = p.msd && !r.msd_ok;
    if (msd_missed && (r.msd_flags & 4u) == 0u) {
      // a bucket above the finish kernel's capacity: the window was too coarse for this data -- typically fitted to another
      // scene: forget the older frames' ranges -- or the data has > GGD_MSD_CAP equal keys, which no window cures: the pause doubles
      msd_oversize_streak = msd_oversize_streak < 4 ? msd_oversize_streak + 1 : 4;
      msd_ban = GGD_MSD_BAN >> (4 - msd_oversize_streak);
      win_n = 0; win_pos = 0;
    } else if (msd_missed) {
      msd_ban = 2;   // a key outside the window: this frame's range joins the ring below, the next windows contain it
    }
    if (r.folded && r.kmin <= r.kmax) {
      win_lo[win_pos] = r.kmin; win_hi[win_pos] = r.kmax;
      win_pos = (win_pos + 1) % GGD_MSD_WIN;
      if (win_n < (1 << 30)) win_n += 1;
    }
    if (p.msd && !msd_missed) { msd_frames += 1; msd_oversize_streak = 0; }
    const bool again = !abandoned && (msd_missed || (three && !r.flat));
    if (again) reruns += 1;
    return again;
  }
};
