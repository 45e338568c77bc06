// ggd_common.h -- shared declarations of the gfx950 rasterizer library (host ctx + device helpers).
//
// Arithmetic contract: every translation unit is compiled with -ffp-contract=off, so an fp32 expression written
// here is evaluated as written (IEEE mul/add/div/sqrt, correctly rounded) unless it says __builtin_fmaf
// explicitly.  The per-Gaussian stage keeps the operation order of the algorithm's published form so that its
// integer outputs (radii, tiles_touched, depth bits -> sort keys) are reproducible bit-for-bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>

#include "ggd_raster.h"
#include "ggd_spec.h"
#include "ggd_binning_layout.h"

#define GGD_WAVE 64

// Stage ids for the optional hipEvent profiler (ggd_set_profiling).
enum {
  ST_PREPROCESS = 0, ST_SCAN, ST_READBACK, ST_DUPLICATE, ST_SORT, ST_RANGES, ST_BLEND,
  ST_BLEND_BWD, ST_PREPROCESS_BWD, ST_COUNT
};

enum { GGD_ATTR_MLP_FWD = 1, GGD_ATTR_MLP_BWD = 2, GGD_ATTR_MLP_WGRAD = 4, GGD_ATTR_MLP_HL = 64 };

// layout of the debug statistics buffer of the forward blend (ggd_blend_stats / ggd_blend_timeline)
constexpr int GGD_STATS_MODE = 9;            // word: 0 = counters (atomics), 1 = per-wave timeline slots
constexpr int GGD_STATS_BWD = 16;            // eight counters of the backward blend (quarter form), see blend_backward_quarter_kernel
constexpr int GGD_STATS_HEAD = 32;           // first timeline slot (3 words per wave: start, end, listed << 32 | gathered)
constexpr int GGD_STATS_MAX_WAVES = 1 << 17;

// (two-launch depth sort: described at ggd_fold below; GGD_MSD_BINS / CAP / MAX_TILES are in ggd_binning_layout.h, the constants
// the host's policy needs in ggd_spec.h)

// One frame's arguments as the entry points of the C ABI receive them, in four groups: each entry point of ggd_capi.hip fills them
// once, field by name, and everything below it -- the host functions there, the launchers declared at the end of this file -- takes
// the groups.  Host only: no kernel receives one.  Every field has a default: a group filled in part is well defined.
struct ggd_inputs {       // [P, ...] fp32 each; which may be NULL: check_inputs (ggd_capi.hip)
  const float *means3D = nullptr, *shs = nullptr, *colors_precomp = nullptr, *opacities = nullptr;
  const float *scales = nullptr, *rotations = nullptr, *cov3D_precomp = nullptr;
};
struct ggd_frame_bufs {   // the caller's buffers of one forward frame
  void* geom_buf = nullptr; int32_t* radii = nullptr;
  void* binning_buf = nullptr; int64_t capacity = 0;   // capacity: instances binning_buf was laid out for (ggd_binning_layout), >= the R processed
  void* img_buf = nullptr;
  float *out_color = nullptr, *out_depth = nullptr, *out_alpha = nullptr;   // depth / alpha: the *_aux entry points' planes (both or neither)
};
struct ggd_pix_grads {    // the backward's incoming gradients: [3, H, W] and, NULL = zero, [H, W] each
  const float *dL_dpix = nullptr, *dL_ddepth = nullptr, *dL_dalpha = nullptr;
};
struct ggd_grads {        // the backward's results, each written in full by the library
  float *dL_dmeans2D = nullptr, *dL_dcolors = nullptr, *dL_dopacity = nullptr, *dL_dmeans3D = nullptr, *dL_dcov3D = nullptr;
  float *dL_dsh = nullptr, *dL_dscales = nullptr, *dL_drots = nullptr;
  float* dL_dmeans2D_abs = nullptr;   // ggd_backward_abs only: [P, 3] = (accumulator slots GGD_ACC_ABS, 0), zeros for culled Gaussians
};

// The frame in flight: what geometry_enqueue leaves for render_enqueue, and render_enqueue for the collection of num_rendered.
// A frame begins in geometry_enqueue, which assigns a fresh one (only the tag carries over); nothing else clears these.
struct ggd_frame {
  // geometry_enqueue -> the first render_enqueue behind it, which takes them (a second render of the same geometry rides on nothing)
  struct {
    bool ride = false;            // the offsets scan was left to the depth sort's launches
    bool folded = false;          // ... and the preprocess built the sort's histograms + the scan's first step (ggd_fold below)
    bool sortctl_clean = false;   // the preprocess cleared ctx->sortctl and no sort has used it since
  } geom;
  ggd_spec_plan plan;             // decided before the preprocess launch
  // render_enqueue -> collection
  bool three_passes = false;      // the fourth sort pass was not launched
  bool r_pending = false;         // the host waits for the tagged word (h_words[2..3]), not for the end of the frame
  uint32_t r_tag = 0;             // ... which carries this sequence number (30 bits, never 0)
  ggd_spec_report report;         // `folded` by render_enqueue, the rest read with num_rendered (the key range only when folded)
};

struct ggd_ctx {
  int device = 0;
  int cus = 0;                  // compute units of the device (sizes the persistent preprocess grid)
  void* scratch = nullptr;      // grow-only device workspace (sort histograms, scan block sums, dL_dconic, ...)
  size_t scratch_bytes = 0;
  uint32_t attr_mask = 0;       // GGD_ATTR_* bits: kernels whose dynamic-LDS limit was raised on this ctx's device
  uint32_t* d_words = nullptr;  // small device control block: [0] total R, [1] prefilter trap flag
  uint32_t* h_words = nullptr;  // pinned host mirror
  uint32_t* h_words_dev = nullptr;  // the same memory as the device sees it (the scan writes num_rendered there itself)
  uint32_t* sortctl = nullptr;      // depth sort's control block (histograms, tickets, kept-key count) in its own allocation
  uint32_t* scan_sums = nullptr;    // block sums of a scan that rides on the depth sort (own allocation, grow-only)
  size_t scan_sums_cap = 0;
  // depth-sort front end folded into the preprocess kernel (ggd_fold below): two control blocks used alternately
  uint32_t* foldctl[2] = {nullptr, nullptr};
  size_t foldctl_cap = 0;           // words per block
  size_t foldctl_dirty[2] = {0, 0}; // words of each block its last user may have written (what the next clear must cover)
  int fold_cur = 0;                 // block the next folding preprocess accumulates into (cleared by the previous one)
  bool fold_poisoned = false;       // a folding launch failed: nothing is known about the blocks -- clear both before the next use
  unsigned long long scan_in_scatter_frames = 0;   // GGD_STAT_SCAN_IN_SCATTER_FRAMES
  unsigned long long l1_counted_frames = 0;        // GGD_STAT_L1_COUNTED_FRAMES
  ggd_spec spec;                    // cross-frame speculation policy: three sort passes / the two-launch sort (ggd_spec.h)
  ggd_frame frame;                  // the one frame in flight
  // ggd_forward_enqueue ... ggd_forward_collect: the frame whose num_rendered has not been collected yet
  struct { bool valid = false; ggd_params prm; ggd_frame_bufs bufs; } pending;
  void* gelu_tables = nullptr;      // GELU / GELU' interpolation tables of the reference-precision decoder kernels (built on first use)
  void *dbg_keys = nullptr, *dbg_vals = nullptr;   // debug copy of the unsorted list
  size_t dbg_cap = 0;
  int opt[GGD_OPT_COUNT] = {3, 1, 1, 1, 1, 1, 0, 1};  // exp: bare v_exp_f32 in the forward blend, compensated 2^x (1-2 ulp) in the backward
  unsigned long long* blend_stats = nullptr;  // debug: device counters filled by the forward blend when non-null
  unsigned long long* stats_buf = nullptr;    // its storage: [0..5] counters, [GGD_STATS_MODE] 1 = per-wave timeline, slots from GGD_STATS_HEAD
  bool profiling = false;
  hipEvent_t ev[2 * ST_COUNT] = {};
  bool ev_used[ST_COUNT] = {};
  std::string err;
};

// The offsets scan of stage a5 as a passenger of the depth sort (single-call forward): its three steps are run by extra
// workgroups appended to the sort's histogram / pass-0 / pass-1 launches -- each step only depends on the previous
// launch, and nothing on the tile-binning paths reads the offsets or the total before the frame ends -- so the scan
// costs no launches of its own (three launches of ~4.8 us each otherwise).
struct ggd_scan_piggy {
  const uint32_t* in = nullptr;   // tiles_touched[n]
  uint32_t* out = nullptr;        // point_offsets[n] (inclusive)
  int64_t n = 0;
  int nb = 0;                     // ggd_scan_blocks(n)
  uint32_t* block_sums = nullptr; // [nb] scratch
  uint32_t* d_total = nullptr;    // device word for the grand total (num_rendered)
  uint32_t* h_total = nullptr;    // device view of the pinned host word (may be NULL)
  unsigned long long* h_tagged = nullptr;   // device view of a pinned 64-bit word that receives (tag << 32 | total): the host
  uint32_t tag = 0;                         // polls it instead of waiting on an event (an event record between two kernels
                                            // costs the GPU a ~6 us bubble)
  // folded front end (ggd_fold): step 1 was done by the preprocess workgroups (256 points each) -- step 2 scans their sums
  const uint4* wg_info = nullptr;           // [n_info] {sum of tiles_touched, kept depth keys, ~min kept key, max kept key} per 256-Gaussian tile of the preprocess
  int n_info = 0;
  uint32_t* n_valid = nullptr;              // receives the number of kept keys (sum of wg_info[].y)
  int sum_stride = 1;                       // block_sums entries per scan block of step 3 (8 with wg_info: 2048 / 256)
  uint32_t* flat_flag = nullptr;            // folded front end: "the order is in the third pass's output" word of the consumers
  int spec_flat = 0;                        // != 0: only three passes were launched -- set *flat_flag whatever the histogram says
  uint32_t* fold_hist = nullptr;            // the folded front end's histogram replicas: the workgroup that runs step 2 also adds
                                            // replicas 1 .. REPS-1 of passes 1 .. 3 into replica 0 (only pass 0 reads them all)
  int msd = 0;                              // unused, kept for the kernarg layout
  uint32_t msd_lo = 0;                      // unused, kept for the kernarg layout
  int msd_shift = GGD_MSD_SHIFT;            // unused, kept for the kernarg layout
};

// The depth sort's histogram kernel folded into the preprocess kernel (single-call forward on the tile-binning path): every
// preprocess workgroup adds the digit counts of its kept depth keys to one of GGD_FOLD_REPS replicas of the four 256-bin
// histograms and stores {sum of tiles_touched, kept keys} of its 256 points -- the histogram launch (19 us at 1 M points:
// its 245 workgroups flush into the same 64 lines, and atomic instructions on one line serialise at ~43 ns per 16 lanes) and
// step 1 of the offsets scan disappear.  The control block ("fold block": GGD_FOLD_REPS replicas of the histograms, the sort's
// control words, the row totals, every status word) is laid out in ggd_binning_layout.h; two blocks alternate, each cleared by
// the preprocess of the frame before its use.
// Two-launch depth sort (round 5; `msd` in ggd_fold / ggd_scan_piggy; the key WINDOW since round 6).  The kept keys of a frame lie
// in a narrow range of the 32-bit key space (fp32 bits of depths between, say, 1.8 and 3.6): over a window [lo, lo + 1024 << shift)
// that contains them they are ordered by ONE most-significant-digit partition and an in-LDS finish instead of three or four
// onesweep passes with their cross-tile look-back (48 -> see DESIGN.md):
//   launch 1  every 4096-key tile partitions ITS OWN keys by bucket = (key - lo) >> shift (1024 buckets, stable, culled keys
//             dropped), writes (key - lo, index) to its own region and a table {offset, count} per (tile, bucket) -- no dependency
//             between tiles at all;
//   launch 2  one 1024-thread workgroup per bucket gathers the bucket's pieces from all tiles in tile order (= index order),
//             orders them by the `shift` low bits of (key - lo) with (up to) two stable 8-bit counting passes in LDS and writes
//             the run of indices to its final place (bucket bases = prefix of the preprocess kernel's 1024-bin histogram).
// Round 5 fixed the window to one binade pair (bucket = key bits 14..23, precondition: a constant top byte).  That fails for a
// depth range that straddles 2.0 -- which the reference's pose sampler produces (camera.py:6-35: radius 2.7, yaw +- 1 rad: the
// unit cube's near corner comes to depth 1.83) -- and left a head-like scene's keys in 154 of the 1024 buckets.  Now the host
// fits the window to the ranges of the last GGD_MSD_WIN folded frames (+ 1/8 margin either side; every frame's kept-key min / max
// arrive with num_rendered) and the shift to the window (<= GGD_MSD_MAX_SHIFT: two 8-bit passes).  (2048 buckets were measured
// in round 5: launch 1 pays + 3 us for the wider digit, profiles/REJECTED.md.)
// The host speculates (after GGD_FLAT_STREAK folded frames); the frame's own front end verifies (no kept key outside the window:
// GGD_FOLD_OUTSIDE == 0; no bucket above GGD_MSD_CAP) and a frame that fails is binned and blended again by the ordinary path (as
// for the skipped fourth pass); a key outside the window is clamped into the last bucket, so the kernels behind always see a
// valid permutation.
// (The kept keys' range of a frame -- what the two-launch sort's window is fitted to -- travels with the per-workgroup sums in
// wg_info, as plain stores.  Round 6's first forms kept {~min, max} replicas here, updated with atomicMax: 16 replicas packed into
// two 64-byte lines cost the preprocess kernel + 30 us (atomics on one line serialise at ~11 ns), one line per replica behind a
// read-and-compare still + 10 us: a device-scope load + atomic at the END of every workgroup adds 2 - 4 us to its ~8 us lifetime.)
struct ggd_fold {
  uint32_t* ctl = nullptr;        // this frame's control block (clean)
  uint32_t* clear = nullptr;      // the other block ...
  uint32_t clear_words = 0;       // ... and how much of it the preprocess clears for the next frame
  uint4* wg_info = nullptr;       // [ceil(P / 256)] {sum of tiles_touched, kept keys, ~min kept key, max kept key} per 256-Gaussian tile
  int rows = 0;                   // != 0: also count the Gaussians per tile row (the grid has <= 64 rows)
  uint32_t* rowinst = nullptr;    // ... and the instances per tile row, in REPS x 64 words of ctl (ggd_fold_rowinst)
  int msd = 0;                    // != 0: histograms of the two-launch sort (1024 buckets of the key window, top byte) instead of the four bytes
  uint32_t msd_lo = 0;            // bucket of a kept key = min((key - msd_lo) >> msd_shift, 1023); a key for which the unclamped
  int msd_shift = GGD_MSD_SHIFT;  // value exceeds 1023 (below the window: the difference wraps) is counted in GGD_FOLD_OUTSIDE
};

int ggd_fail(ggd_ctx* ctx, int code, const std::string& msg);
int ggd_reserve_scratch(ggd_ctx* ctx, size_t bytes, hipStream_t stream);

static inline const char* ggd_basename(const char* p) {
  const char* b = p;
  for (; *p; ++p) if (*p == '/') b = p + 1;
  return b;
}
#define GGD_HIP(call)                                                                                      \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess)                                                                                  \
      return ggd_fail(ctx, GGD_E_HIP, std::string(#call) + " (" + ggd_basename(__FILE__) + ":" +            \
                                          std::to_string(__LINE__) + "): " + hipGetErrorString(e_));         \
  } while (0)

struct StageTimer {  // RAII hipEvent pair around one pipeline stage (no-op unless profiling is on)
  ggd_ctx* c; int st; hipStream_t s;
  StageTimer(ggd_ctx* ctx, int stage, hipStream_t stream) : c(ctx), st(stage), s(stream) {
    if (c->profiling) { (void)hipEventRecord(c->ev[2 * st], s); }
  }
  ~StageTimer() {
    if (c->profiling) { (void)hipEventRecord(c->ev[2 * st + 1], s); c->ev_used[st] = true; }
  }
};

// Runtime value -> template argument, for the launchers: calls f(std::integral_constant<int, I>{}) with I = v for
// 0 <= v < N - 1 and I = N - 1 for every other v (a bool is N = 2).  Kernel templates take their feature flags as trailing
// defaulted parameters (preprocess_kernel<..., AA>, blend_forward_kernel<..., AUX>, ...): one definition per kernel, the
// plain instance is <..., false>, and a launcher names the instance inside nested ggd_dispatch calls around ONE launch.
template <int N, int I = 0, typename F>
static inline void ggd_dispatch(int v, F&& f) {
  if constexpr (I == N - 1) f(std::integral_constant<int, I>{});
  else if (v == I) f(std::integral_constant<int, I>{});
  else ggd_dispatch<N, I + 1>(v, f);
}

// ---- kernels launched by the C API (defined in the .hip files) ------------------------------------------------
int ggd_launch_preprocess(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_inputs& in, ggd_splat* splat,
                          uint32_t* tiles_touched, uint8_t* clamped, int32_t* radii,
                          uint32_t* depth_keys, uint2* rect, uint32_t* trap_flag, uint32_t* zero_ptr = nullptr,
                          int zero_words = 0,    // zero_words words at zero_ptr are cleared by the first workgroups
                          const ggd_fold* fold = nullptr);
int ggd_launch_mark_visible(ggd_ctx* ctx, hipStream_t s, int P, const float* means3D, const float* view,
                            uint8_t* present);
// inclusive scan of a uint32 array; total written to *d_total (device) and, if given, to h_total (device view of a pinned
// host word)
int ggd_launch_inclusive_scan(ggd_ctx* ctx, hipStream_t s, const uint32_t* in, uint32_t* out, int64_t n,
                              uint32_t* d_total, void* tmp, size_t tmp_bytes, uint32_t* h_total = nullptr);
size_t ggd_scan_tmp_bytes(int64_t n);
int ggd_scan_blocks(int64_t n);   // workgroups (= block sums) of the scan over n elements
int ggd_launch_duplicate(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const uint2* rect,
                         const uint32_t* depth_keys, const uint32_t* tiles_touched, const uint32_t* offsets,
                         uint64_t* keys, uint32_t* vals);
// (tmp sizes, the control block and its device words -- kept keys, "flat" -- : ggd_binning_layout.h, ggd_sort_ctl)
// stable LSD radix sort of (key,val) pairs on key bits [0,nbits); result ends in (keys_a, vals_a); the input must
// have been placed in the buffer ggd_sort_input_is_alt(nbits) says.
int ggd_sort_input_is_alt(int nbits);
int ggd_launch_sort(ggd_ctx* ctx, hipStream_t s, uint64_t* keys_a, uint32_t* vals_a, uint64_t* keys_b,
                    uint32_t* vals_b, int64_t n, int nbits, void* tmp, size_t tmp_bytes);
// 32-bit-key variant (depth sort of the Gaussians).  keys_src is only read; the result ends in (keys_a, vals_a);
// values start as the identity permutation.  nbits must be a multiple of 16 (even number of passes).
struct ggd_sort32_opts {
  uint32_t* clean_ctl = nullptr;           // a control block (ggd_sort_ctrl_words) an earlier kernel of the frame has cleared: no memset launch
  const ggd_scan_piggy* piggy = nullptr;   // an offsets scan that rides on the sort's launches
  const ggd_fold* fold = nullptr;          // histograms, kept-key count and the scan's step 1 come from the preprocess kernel (piggy must
                                           // carry wg_info); no histogram launch.  The workgroup that runs the scan's step 2 reports "top
                                           // digit constant" in bit 63 of the tagged num_rendered word and in d_total[2].
  bool flag_flat_last = false;             // a constant-digit LAST pass copies nothing -- it sets ggd_sort_ctl::flat and the result stays in
                                           // (keys_b, vals_b)
  bool apply_here = true;                  // false: the caller runs the riding scan's last step (offsets) elsewhere -- ggd_launch_rowbin(apply = ...)
  bool skip_last = false;                  // (fold only) the last pass is not launched (the caller expects a constant top digit); the
                                           // consumers' flat word is set regardless, so that they read the third pass's output (a valid
                                           // permutation either way)
};
int ggd_launch_sort32_iota(ggd_ctx* ctx, hipStream_t s, const uint32_t* keys_src, uint32_t* keys_a, uint32_t* vals_a,
                           uint32_t* keys_b, uint32_t* vals_b, int64_t n, int nbits, void* tmp, size_t tmp_bytes,
                           const ggd_sort32_opts& opts = ggd_sort32_opts());
bool ggd_sort32_msd_supported(int64_t n);
// Counted level 1 of the row binning (GGD_OPT_L1_COUNTED; grids of <= 64 x 64 tiles behind the two-launch sort): the finish launch,
// which holds every bucket in its final order, also gathers the rects and counts the row entries of its bucket -- per bucket and
// in front of every 1024-rank chunk boundary inside it -- so that rb_level1_counted_kernel sums finished rows instead of looking
// back over the chunks of its own launch.  The three arrays live in the row binning's scratch (ggd_rowbin_counted).
struct ggd_l1_counted {
  const uint2* rect = nullptr;        // [P] tile rect of every Gaussian (the preprocess kernel's)
  uint2* packed = nullptr;            // [P] by depth rank: {id, x0 | x1 << 8 | y0 << 16 | y1 << 24}, zeros for an empty rect
  uint32_t* bucket_rows = nullptr;    // [GGD_MSD_BINS][64]
  uint32_t* boundary_rows = nullptr;  // [chunks][64]
  int chunks = 0;                     // rb_blocks1(P)
};
int ggd_launch_sort32_msd(ggd_ctx* ctx, hipStream_t s, const uint32_t* keys_src, uint32_t* keys_a, uint32_t* vals_a,
                          uint32_t* keys_b, uint32_t* vals_b, int64_t n, uint32_t* table, const ggd_scan_piggy* piggy,
                          const ggd_fold* fold, const ggd_l1_counted* counted = nullptr);
// Tile binning (GGD_OPT_BINNING = 1): sorted Gaussian order -> per-tile lists + ranges.
bool ggd_rowbin_supported(int W, int H);
static inline size_t ggd_rowbin_tmp_bytes(int P, uint32_t capacity, int W, int H) { return ggd_rowbin_layout(P, capacity, W, H).total_counted; }
// the counted level 1's arrays inside the row binning's scratch (narrow grids only; tmp holds ggd_rowbin_tmp_bytes)
static inline ggd_l1_counted ggd_rowbin_counted(void* tmp, const uint2* rect, int P, uint32_t capacity, int W, int H) {
  const ggd_rowbin_tmp lay = ggd_rowbin_layout(P, capacity, W, H);
  char* p = static_cast<char*>(tmp);
  ggd_l1_counted c;
  c.rect = rect; c.packed = reinterpret_cast<uint2*>(p + lay.packed);
  c.bucket_rows = reinterpret_cast<uint32_t*>(p + lay.bucket_rows);
  c.boundary_rows = reinterpret_cast<uint32_t*>(p + lay.boundary_rows);
  c.chunks = rb_blocks1(P);
  return c;
}
struct ggd_rowbin_opts {
  const uint32_t *order_alt = nullptr, *use_alt = nullptr;   // *use_alt != 0 (device): the depth order is in order_alt (ggd_launch_sort32_iota)
  const ggd_scan_piggy* apply = nullptr; // step 3 of a riding scan, as appended workgroups of the last (longest) binning launch
  // folded front end, grids of <= 64 x 64 tiles (all three or none): the preprocess kernel counted the entries per tile row -- level 1 is
  // ONE launch (count, look-back, scatter) -- and the instances per tile row -- level 2's scatter forms its tile starts itself (no scan launch)
  struct { const uint32_t* rowtot = nullptr; uint32_t* status1 = nullptr; const uint32_t* rowinst = nullptr; } fold;   // ggd_fold_rowtot, ..
  const uint32_t* counted_hist = nullptr;   // (with fold; grids of <= 64 x 64 tiles) the two-launch sort's bucket histogram -- its finish
                                            // launch was given ggd_rowbin_counted(tmp, ...) and level 1 runs without its look-back
};
struct ggd_rowbin_result {
  int rc = GGD_OK;
  bool scan_in_scatter = false;   // level 2 ran without its scan launch
};
ggd_rowbin_result ggd_launch_rowbin(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const uint2* rect, const uint32_t* order,
                                    const uint32_t* n_vis_ptr, uint32_t* list, uint32_t* ranges, uint32_t capacity, void* tmp,
                                    size_t tmp_bytes, const ggd_rowbin_opts& opts = ggd_rowbin_opts());
int ggd_launch_ranges(ggd_ctx* ctx, hipStream_t s, const uint64_t* keys, int64_t n, uint32_t* ranges, int T);
// the cross-lane primitives of ggd_lanes.h next to their __shfl forms (ggd_selftest_lanes, ggd_raster.h)
int ggd_launch_selftest_lanes(ggd_ctx* ctx, hipStream_t s, const uint64_t* in, uint32_t* out, int n_waves);
// out_depth / out_alpha non-null (both): the depth / alpha extension (blend_forward_kernel<..., AUX>), which also reads
// depth_keys (the geometry buffer's: the fp32 bits of each Gaussian's view-space depth)
int ggd_launch_blend(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                     const uint32_t* list, const uint32_t* ranges, uint32_t capacity, float* out_color, float* final_T,
                     uint32_t* n_contrib, const uint32_t* depth_keys = nullptr, float* out_depth = nullptr,
                     float* out_alpha = nullptr);
// Backward accumulator record (library scratch, one per Gaussian, zeroed with ONE memset): the blend backward adds its
// per-(tile, Gaussian) sums here, the per-Gaussian backward reads it once and writes every caller-visible gradient
// (zeros for culled Gaussians), so the caller's 8 gradient arrays need no zero-fill passes.
constexpr int GGD_ACC_FLOATS = 12;   // 48 B: conic A,B,C | opacity | mean2D x,y | colour r,g,b | depth (aux only) | abs mean2D x,y
constexpr int GGD_ACC_CONIC = 0, GGD_ACC_OPACITY = 3, GGD_ACC_MEAN2D = 4, GGD_ACC_COLOR = 6;
constexpr int GGD_ACC_DEPTH = 9;     // dL/dz (view-space depth), written only by the depth / alpha and the distortion backward
constexpr int GGD_ACC_ABS = 10;      // sum over pixels of |d/d mean2D x|, |.. y| (slots 10, 11), written only by an absgrad backward
// aux: the depth / alpha backward (blend_backward_quarter_kernel<..., AUX>, always the quarter form); depth_keys as in
// ggd_launch_blend, pix.dL_ddepth / pix.dL_dalpha [H, W] (NULL = zero; read only when aux).  abs: the absolute screen-space
// gradient sums as well (slots GGD_ACC_ABS; quarter form only, with or without aux)
int ggd_launch_blend_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                              const uint32_t* list, const uint32_t* ranges, const float* final_T,
                              const uint32_t* n_contrib, const ggd_pix_grads& pix, float* grad_acc /*[P][GGD_ACC_FLOATS]*/,
                              bool aux, const uint32_t* depth_keys, bool abs);
// Feature maps (ggd_features.hip; ggd_forward_features / ggd_backward_features): C channels per Gaussian blended over the
// contributors of a finished colour render.  R: the forward's num_rendered (the list's length); n_contrib / final_T: the image
// buffer's.  The backward ADDS its conic / opacity / mean2D sums to the accumulator records (between the blend backward and the
// per-Gaussian backward) and its feature gradients to dL_dfeatures [P, C], which the caller has zero-filled.
int ggd_launch_features_forward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                const uint32_t* list, const uint32_t* ranges, uint32_t R, const uint32_t* n_contrib,
                                const float* features, int C, const float* feature_bg /*NULL = 0*/, float* out /*[C, H, W]*/);
int ggd_launch_features_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                 const uint32_t* list, const uint32_t* ranges, uint32_t R, const float* final_T,
                                 const uint32_t* n_contrib, const float* features, int C, const float* feature_bg,
                                 const float* dL_dF /*[C, H, W]*/, float* grad_acc, float* dL_dfeatures /*[P, C]*/);
// Distortion map (ggd_distortion.hip; ggd_forward_distortion / ggd_backward_distortion): D = sum_ij w_i w_j |z_i - z_j| over the
// contributors of a finished colour render, z from depth_keys as in ggd_launch_blend.  The backward ADDS its conic / opacity /
// mean2D sums and dL/dz (slot GGD_ACC_DEPTH) to the accumulator records, where the feature blend's backward adds its own.
int ggd_launch_distortion_forward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                  const uint32_t* list, const uint32_t* ranges, uint32_t R, const uint32_t* n_contrib,
                                  const uint32_t* depth_keys, float* out /*[H, W]*/);
int ggd_launch_distortion_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                   const uint32_t* list, const uint32_t* ranges, uint32_t R, const float* final_T,
                                   const uint32_t* n_contrib, const uint32_t* depth_keys, const float* dL_dD /*[H, W]*/,
                                   float* grad_acc);
// Contribution statistics (ggd_contribution.hip; ggd_contribution): per Gaussian the fixed-point sum, the count and the maximum of
// w = alpha T over the (pixel, record) pairs of a finished colour render, ACCUMULATED into stats [P][3] with integer atomics.
int ggd_launch_contribution(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat, const uint32_t* list,
                            const uint32_t* ranges, uint32_t R, const uint32_t* n_contrib, int64_t* stats /*[P][3]*/);
// aux: also adds dL/dz (accumulator slot GGD_ACC_DEPTH) times dz/dmean = (view[2], view[6], view[10]) to dL_dmeans3D
// out.dL_dmeans2D_abs non-null: the absgrad kernels, which write it too
int ggd_launch_preprocess_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_inputs& in,
                                   const int32_t* radii, const uint8_t* clamped, const float* grad_acc, const ggd_grads& out,
                                   bool aux);
// Camera gradients (ggd_camera.hip; ggd_backward_camera): behind the per-Gaussian backward, on the same accumulator records and
// inputs.  partial: ggd_camera_tmp_bytes(P) of workspace (one row of sums per workgroup); all 35 values of `out` are written.
size_t ggd_camera_tmp_bytes(int P);
int ggd_launch_camera_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_inputs& in, const int32_t* radii,
                               const uint8_t* clamped, const float* grad_acc, bool aux, float* partial,
                               const ggd_camera_grads& out);

// ---- device helpers -----------------------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ int ggd_tile_rect(float px, float py, int irad, int gx, int gy, int& minx, int& miny,
                                             int& maxx, int& maxy) {
  // C-style truncation of (p -/+ r [+15]) / 16, clamped to the tile grid.  float->int saturates on gfx950.
  const float fr = (float)irad;
  minx = min(gx, max(0, (int)((px - fr) / 16.0f)));
  miny = min(gy, max(0, (int)((py - fr) / 16.0f)));
  maxx = min(gx, max(0, (int)((px + fr + 15.0f) / 16.0f)));
  maxy = min(gy, max(0, (int)((py + fr + 15.0f) / 16.0f)));
  return (maxx - minx) * (maxy - miny);
}
#endif
