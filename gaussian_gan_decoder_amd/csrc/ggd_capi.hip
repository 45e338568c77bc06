// ggd_capi.hip -- the C ABI declared in include/ggd_raster.h (host side: ctx, workspace, stage sequencing).
//
// A single-call frame on the tile-binning path (ggd_forward, ggd_forward_enqueue) is enqueued whole before the host knows
// num_rendered -- binning_buf's capacity stands in for it -- in seven launches when the two-launch sort is planned:
//   geometry_enqueue  preprocess; with GGD_OPT_FOLD it also builds the depth sort's histograms (which ones: this frame's plan,
//                     ggd_spec.h), step 1 of the offsets scan and the binning's entries and instances per tile row (ggd_fold)
//   render_enqueue    depth sort (two launches over the planned key window, or three / four onesweep passes), row / column binning,
//                     blend; steps 2 and 3 of the scan ride on the sort's first and the binning's last launch
//   collect           the ONE host wait: geometry_finish polls the pinned word (flags | tag | num_rendered) that scan step 2 stores
//                     and returns while binning and blend still run.  Flags + kept-key range are the frame's report to the policy;
//                     a frame whose short sort did not hold is rendered again from its geometry buffer: depth sort with its own
//                     histogram launch and four passes, binning, blend -- no second preprocess
// The frame in flight (ggd_frame) is assigned fresh where a frame begins, in geometry_enqueue, and where it is collected.
// Every other frame: preprocess -> scan -> read-back of num_rendered (a stream synchronise) -> either binning path -> blend.
// (Below the extern "C" entry points the arguments travel in the groups of ggd_common.h: ggd_inputs, ggd_frame_bufs, ...)
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <new>

#include "ggd_common.h"

static std::string g_create_error;

static const char* const kStageNames[ST_COUNT] = {"preprocess", "scan", "readback", "duplicate", "sort",
                                                  "ranges", "blend", "blend_bwd", "preprocess_bwd"};

int ggd_fail(ggd_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg; else g_create_error = msg;
  return code;
}

int ggd_reserve_scratch(ggd_ctx* ctx, size_t bytes, hipStream_t stream) {
  if (bytes <= ctx->scratch_bytes) return GGD_OK;
  // grow-only with head-room so steady-state training never reallocates
  size_t want = bytes + bytes / 4 + (1u << 20);
  if (ctx->scratch) {
    GGD_HIP(hipStreamSynchronize(stream));
    GGD_HIP(hipFree(ctx->scratch));
    ctx->scratch = nullptr; ctx->scratch_bytes = 0;
  }
  hipError_t e = hipMalloc(&ctx->scratch, want);
  if (e != hipSuccess) return ggd_fail(ctx, GGD_E_NOMEM, std::string("hipMalloc scratch: ") + hipGetErrorString(e));
  ctx->scratch_bytes = want;
  return GGD_OK;
}

// ---- layouts -------------------------------------------------------------------------------------------------
extern "C" int ggd_geom_layout(int32_t P, ggd_geom_view* v) {
  if (!v || P < 0) return GGD_E_INVALID;
  size_t off = 0;
  v->splat = off; off += ggd_align((size_t)P * sizeof(ggd_splat));
  v->tiles_touched = off; off += ggd_align((size_t)P * sizeof(uint32_t));
  v->point_offsets = off; off += ggd_align((size_t)P * sizeof(uint32_t));
  v->clamped = off; off += ggd_align((size_t)P);
  v->depth_keys = off; off += ggd_align((size_t)P * sizeof(uint32_t));
  v->rect = off; off += ggd_align((size_t)P * 2 * sizeof(uint32_t));
  v->header = off; off += (P > 0 ? 256 : 0);
  v->total = off;
  return GGD_OK;
}
extern "C" int ggd_binning_layout(int64_t R, ggd_binning_view* v) {
  if (!v || R < 0) return GGD_E_INVALID;
  size_t off = 0;
  // the sorted list comes first: it is the only part the backward reads, so its position does not depend on the R
  // the buffer was laid out for (a capacity in the single-call forward, num_rendered in the two-call form)
  v->list = off; off += ggd_align((size_t)R * sizeof(uint32_t));
  v->list_alt = off; off += ggd_align((size_t)R * sizeof(uint32_t));
  v->keys = off; off += ggd_align((size_t)R * sizeof(uint64_t));
  v->keys_alt = off; off += ggd_align((size_t)R * sizeof(uint64_t));
  v->total = off;
  return GGD_OK;
}
extern "C" int ggd_img_layout(int32_t W, int32_t H, ggd_img_view* v) {
  if (!v || W < 0 || H < 0) return GGD_E_INVALID;
  const size_t T = (size_t)((W + 15) / 16) * ((H + 15) / 16);
  size_t off = 0;
  v->ranges = off; off += ggd_align(T * 2 * sizeof(uint32_t));
  v->final_T = off; off += ggd_align((size_t)W * H * sizeof(float));
  v->n_contrib = off; off += ggd_align((size_t)W * H * sizeof(uint32_t));
  v->total = off;
  return GGD_OK;
}
extern "C" size_t ggd_geom_bytes(int32_t P) { ggd_geom_view v; return ggd_geom_layout(P, &v) == GGD_OK ? v.total : 0; }
extern "C" size_t ggd_binning_bytes(int64_t R) { ggd_binning_view v; return ggd_binning_layout(R, &v) == GGD_OK ? v.total : 0; }
extern "C" size_t ggd_img_bytes(int32_t W, int32_t H) { ggd_img_view v; return ggd_img_layout(W, H, &v) == GGD_OK ? v.total : 0; }

static uint32_t higher_msb(uint32_t n) {  // smallest k with (n >> k) == 0, by bisection from 16
  uint32_t msb = 16, step = 16;
  while (step > 1) {
    step /= 2;
    if (n >> msb) msb += step; else msb -= step;
  }
  if (n >> msb) msb++;
  return msb;
}
extern "C" int ggd_sort_bits(int32_t W, int32_t H) {
  const uint32_t T = (uint32_t)((W + 15) / 16) * (uint32_t)((H + 15) / 16);
  return 32 + (int)higher_msb(T);
}

// The binning path of R instances: true = depth sort + row / column binning, false = duplicate + 64-bit sort + ranges.
// GGD_OPT_BINNING: 0 = the latter; 3 (2: alias) = the former wherever it can run (grids <= 255 x 255 tiles, no debug taps); 1 = auto:
// the same for R > 0 -- since the single-call forward stopped waiting for the end of the frame the binning wins at every size
// measured (18 k instances: 95 vs 123 us per frame, 170 k: 120 vs 158, 1.25 M: 207 vs 296; the threshold used to be 0.79 M).
static bool use_tile_binning(const ggd_ctx* ctx, const ggd_params* prm, int64_t R) {
  const int mode = ctx->opt[GGD_OPT_BINNING];
  return !prm->debug && ggd_rowbin_supported(prm->width, prm->height) && (mode >= 2 || (mode == 1 && R > 0));
}

// Grow-only device buffers that share one capacity (in elements): nothing to do while *cap >= need; else they are freed -- behind
// the stream's work when sync is set -- and allocated again for `want` elements (need + the site's own head-room).
struct ggd_buf { void** ptr; size_t elem; };
static int grow_buffers(ggd_ctx* ctx, std::initializer_list<ggd_buf> bufs, size_t* cap, size_t need, size_t want,
                        const hipStream_t* sync = nullptr) {
  if (*cap >= need) return GGD_OK;
  if (sync) GGD_HIP(hipStreamSynchronize(*sync));
  for (const ggd_buf& b : bufs) { if (*b.ptr) (void)hipFree(*b.ptr); *b.ptr = nullptr; }
  *cap = 0;
  for (const ggd_buf& b : bufs) GGD_HIP(hipMalloc(b.ptr, want * b.elem));
  *cap = want;
  return GGD_OK;
}

// Typed views of the three caller buffers (ggd_geom_layout / ggd_binning_layout / ggd_img_layout).
template <class T> static T* ggd_at(const void* base, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(const_cast<void*>(base)) + off);
}
struct geom_ptrs { ggd_splat* splat; uint32_t *tiles, *offsets; uint8_t* clamped; uint32_t* depth_keys; uint2* rect; };
struct binning_ptrs { uint32_t *list, *list_alt; uint64_t *keys, *keys_alt; };
struct img_ptrs { uint32_t* ranges; float* final_T; uint32_t* n_contrib; };
static geom_ptrs geom_view(const ggd_params* prm, const void* buf) {
  ggd_geom_view v; ggd_geom_layout(prm->P, &v);
  return {ggd_at<ggd_splat>(buf, v.splat), ggd_at<uint32_t>(buf, v.tiles_touched), ggd_at<uint32_t>(buf, v.point_offsets),
          ggd_at<uint8_t>(buf, v.clamped), ggd_at<uint32_t>(buf, v.depth_keys), ggd_at<uint2>(buf, v.rect)};
}
static binning_ptrs binning_view(int64_t layout_R, const void* buf) {
  ggd_binning_view v; ggd_binning_layout(layout_R, &v);
  return {ggd_at<uint32_t>(buf, v.list), ggd_at<uint32_t>(buf, v.list_alt), ggd_at<uint64_t>(buf, v.keys), ggd_at<uint64_t>(buf, v.keys_alt)};
}
static img_ptrs img_view(int32_t W, int32_t H, const void* buf) {
  ggd_img_view v; ggd_img_layout(W, H, &v);
  return {ggd_at<uint32_t>(buf, v.ranges), ggd_at<float>(buf, v.final_T), ggd_at<uint32_t>(buf, v.n_contrib)};
}

// ---- ctx -----------------------------------------------------------------------------------------------------
extern "C" const char* ggd_version(void) { return "ggd-raster 0.1 (gfx950)"; }
extern "C" int ggd_stage_count(void) { return ST_COUNT; }
extern "C" const char* ggd_stage_name(int s) { return (s >= 0 && s < ST_COUNT) ? kStageNames[s] : ""; }

// Every option, in the order of its number (include/ggd_raster.h): the environment variable that sets it when a context is created
// and its largest value.
static constexpr struct { int option; const char* env; int max; } kOptions[GGD_OPT_COUNT] = {
    {GGD_OPT_EXP_MODE, "GGD_EXP_MODE", 3}, {GGD_OPT_BLEND_CULL, "GGD_BLEND_CULL", 1}, {GGD_OPT_BINNING, "GGD_BINNING", 3},
    {GGD_OPT_BLEND_SPLIT, "GGD_BLEND_SPLIT", 4}, {GGD_OPT_FOLD, "GGD_FOLD", 1}, {GGD_OPT_MSD_SORT, "GGD_MSD_SORT", 1},
    {GGD_OPT_PREPROCESS_WGS, "GGD_PREPROCESS_WGS", GGD_PREPROCESS_WGS_MAX}, {GGD_OPT_L1_COUNTED, "GGD_L1_COUNTED", 1}};
static_assert([] { for (int i = 0; i < GGD_OPT_COUNT; ++i) if (kOptions[i].option != i) return false; return true; }(),
              "kOptions is indexed by the option's number");
static bool option_value_ok(int option, int value) {
  return option >= 0 && option < GGD_OPT_COUNT && value >= 0 && value <= kOptions[option].max;
}

extern "C" ggd_ctx* ggd_create(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    ggd_fail(nullptr, GGD_E_NODEVICE, "no HIP device " + std::to_string(device) + " visible");
    return nullptr;
  }
  ggd_ctx* ctx = new (std::nothrow) ggd_ctx();
  if (!ctx) { ggd_fail(nullptr, GGD_E_NOMEM, "out of host memory"); return nullptr; }
  ctx->device = device;
  for (const auto& d : kOptions) {   // a value out of range is ignored; an on / off option (maximum 1) takes any non-zero number as 1
    const char* e = getenv(d.env);
    const int v = !e ? -1 : (d.max == 1 ? atoi(e) != 0 : atoi(e));
    if (option_value_ok(d.option, v)) ctx->opt[d.option] = v;
  }
  if (const char* e = getenv("GGD_MSD_BUCKETS")) { const int v = atoi(e); if (v >= 16 && v <= GGD_MSD_BINS) ctx->spec.msd_buckets = v; }   // timing experiments
  int prev = 0;
  (void)hipGetDevice(&prev);
  bool ok = hipSetDevice(device) == hipSuccess &&
            hipMalloc((void**)&ctx->d_words, 256) == hipSuccess &&
            // coherent (fine-grained) pinned memory: the tagged num_rendered word must become visible to the polling host
            // while the kernel that stored it is still running, whatever HIP_HOST_COHERENT says
            hipHostMalloc((void**)&ctx->h_words, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess &&
            hipMemset(ctx->d_words, 0, 256) == hipSuccess &&
            hipDeviceGetAttribute(&ctx->cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ctx->cus > 0;
  // stale pinned memory (e.g. of a destroyed context) must never match a tag: r_tag restarts at 1 for every context
  if (ok) memset(ctx->h_words, 0, 64);
  for (int i = 0; ok && i < 2 * ST_COUNT; ++i) ok = hipEventCreate(&ctx->ev[i]) == hipSuccess;
  // device-side view of the pinned mirror (the scan writes num_rendered there itself: no blit for the read-back) and the
  // depth sort's control block in its own allocation (cleared by the scan: no memset launch in front of the sort);
  // both are optional -- without them the forward falls back to the copy / the memset
  if (ok && hipHostGetDevicePointer((void**)&ctx->h_words_dev, ctx->h_words, 0) != hipSuccess) {
    ctx->h_words_dev = nullptr;
    (void)hipGetLastError();
  }
  if (ok && (hipMalloc((void**)&ctx->sortctl, ggd_sort_ctrl_words() * sizeof(uint32_t)) != hipSuccess ||
             hipMemset(ctx->sortctl, 0, ggd_sort_ctrl_words() * sizeof(uint32_t)) != hipSuccess)) {
    ctx->sortctl = nullptr;
    (void)hipGetLastError();
  }
  (void)hipSetDevice(prev);
  if (!ok) {
    ggd_fail(nullptr, GGD_E_HIP, std::string("ggd_create: ") + hipGetErrorString(hipGetLastError()));
    ggd_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

extern "C" void ggd_destroy(ggd_ctx* ctx) {
  if (!ctx) return;
  void* const device_buffers[] = {ctx->scratch, ctx->d_words, ctx->sortctl, ctx->foldctl[0], ctx->foldctl[1], ctx->gelu_tables,
                                  ctx->scan_sums, ctx->stats_buf, ctx->dbg_keys, ctx->dbg_vals};
  for (void* p : device_buffers) if (p) (void)hipFree(p);
  if (ctx->h_words) (void)hipHostFree(ctx->h_words);
  for (int i = 0; i < 2 * ST_COUNT; ++i)
    if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
  delete ctx;
}

extern "C" const char* ggd_last_error(ggd_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

extern "C" int ggd_set_option(ggd_ctx* ctx, int option, int value) {
  if (!ctx) return GGD_E_INVALID;
  if (!option_value_ok(option, value)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_set_option: unknown option or value");
  ctx->opt[option] = value;
  if (option == GGD_OPT_MSD_SORT || option == GGD_OPT_FOLD) {
    // (re)setting the sort options restarts the cross-frame speculation state: the window of recent key ranges, the pause after
    // a miss, the flat-frame streak -- a caller (or a test) that switches forms gets a defined starting point
    ctx->spec.reset();
  }
  return GGD_OK;
}
extern "C" int ggd_blend_stats(ggd_ctx* ctx, int enable, unsigned long long* out) {
  if (!ctx) return GGD_E_INVALID;
  GGD_HIP(hipDeviceSynchronize());
  if (out && ctx->blend_stats) GGD_HIP(hipMemcpy(out, ctx->stats_buf, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (enable) {
    const size_t bytes = (GGD_STATS_HEAD + 3ull * GGD_STATS_MAX_WAVES) * sizeof(unsigned long long);
    if (!ctx->stats_buf) GGD_HIP(hipMalloc((void**)&ctx->stats_buf, bytes));
    GGD_HIP(hipMemset(ctx->stats_buf, 0, bytes));
    if (enable == 2) {   // per-wave timeline instead of the counters
      const unsigned long long one = 1ull;
      GGD_HIP(hipMemcpy(ctx->stats_buf + GGD_STATS_MODE, &one, sizeof(one), hipMemcpyHostToDevice));
    }
    ctx->blend_stats = ctx->stats_buf;
  } else {
    ctx->blend_stats = nullptr;
  }
  return GGD_OK;
}
extern "C" int ggd_blend_backward_stats(ggd_ctx* ctx, unsigned long long* out) {
  if (!ctx || !out) return GGD_E_INVALID;
  if (!ctx->stats_buf) return ggd_fail(ctx, GGD_E_INVALID, "ggd_blend_backward_stats: statistics were never enabled (ggd_blend_stats)");
  GGD_HIP(hipDeviceSynchronize());
  GGD_HIP(hipMemcpy(out, ctx->stats_buf + GGD_STATS_BWD, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return GGD_OK;
}
extern "C" int ggd_blend_timeline(ggd_ctx* ctx, unsigned long long* out, int waves) {
  if (!ctx || !out || waves < 0 || waves > GGD_STATS_MAX_WAVES) return GGD_E_INVALID;
  if (!ctx->stats_buf) return ggd_fail(ctx, GGD_E_INVALID, "ggd_blend_timeline: statistics were never enabled");
  GGD_HIP(hipDeviceSynchronize());
  GGD_HIP(hipMemcpy(out, ctx->stats_buf + GGD_STATS_HEAD, 3ull * waves * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return GGD_OK;
}

extern "C" int ggd_get_option(ggd_ctx* ctx, int option) {
  if (ctx && option == GGD_STAT_FLAT_STREAK) return ctx->spec.flat_streak;
  if (ctx && option == GGD_STAT_SORT_RERUNS) return (int)(ctx->spec.reruns & 0x7fffffffull);
  if (ctx && option == GGD_STAT_MSD_FRAMES) return (int)(ctx->spec.msd_frames & 0x7fffffffull);
  if (ctx && option == GGD_STAT_SCAN_IN_SCATTER_FRAMES) return (int)(ctx->scan_in_scatter_frames & 0x7fffffffull);
  if (ctx && option == GGD_STAT_L1_COUNTED_FRAMES) return (int)(ctx->l1_counted_frames & 0x7fffffffull);
  if (!ctx || option < 0 || option >= GGD_OPT_COUNT) return GGD_E_INVALID;
  return ctx->opt[option];
}

extern "C" int ggd_set_profiling(ggd_ctx* ctx, int enabled) {
  if (!ctx) return GGD_E_INVALID;
  ctx->profiling = enabled != 0;
  for (int i = 0; i < ST_COUNT; ++i) ctx->ev_used[i] = false;
  return GGD_OK;
}

extern "C" int ggd_stage_times(ggd_ctx* ctx, float* ms_out) {
  if (!ctx || !ms_out) return GGD_E_INVALID;
  for (int i = 0; i < ST_COUNT; ++i) {
    ms_out[i] = -1.0f;
    if (ctx->ev_used[i]) {
      GGD_HIP(hipEventSynchronize(ctx->ev[2 * i + 1]));
      float ms = 0.0f;
      GGD_HIP(hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]));
      ms_out[i] = ms;
    }
  }
  return GGD_OK;
}

static int check_params(ggd_ctx* ctx, const ggd_params* prm) {
  if (!ctx) return GGD_E_INVALID;
  if (!prm) return ggd_fail(ctx, GGD_E_INVALID, "params is NULL");
  if (prm->P < 0 || prm->width <= 0 || prm->height <= 0)
    return ggd_fail(ctx, GGD_E_INVALID, "bad P / image size");
  if (!prm->viewmatrix || !prm->projmatrix || !prm->campos || !prm->bg)
    return ggd_fail(ctx, GGD_E_INVALID, "viewmatrix / projmatrix / campos / bg must be device pointers");
  if (prm->sh_degree < 0 || prm->sh_degree > 3) return ggd_fail(ctx, GGD_E_INVALID, "sh_degree must be 0..3");
  if (prm->tanfovx == 0.0f || prm->tanfovy == 0.0f) return ggd_fail(ctx, GGD_E_INVALID, "tanfov must be non-zero");
  return GGD_OK;
}

static int check_inputs(ggd_ctx* ctx, const ggd_params* prm, const ggd_inputs& in) {
  if (prm->P == 0) return GGD_OK;
  if (!in.means3D) return ggd_fail(ctx, GGD_E_INVALID, "means3D is NULL");
  if ((in.shs == nullptr) == (in.colors_precomp == nullptr))
    return ggd_fail(ctx, GGD_E_INVALID, "Please provide excatly one of either SHs or precomputed colors!");
  if (((in.scales == nullptr) || (in.rotations == nullptr)) == (in.cov3D_precomp == nullptr) ||
      ((in.scales == nullptr) != (in.rotations == nullptr)))
    return ggd_fail(ctx, GGD_E_INVALID,
                    "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  if (in.shs && (prm->sh_degree + 1) * (prm->sh_degree + 1) > prm->M)
    return ggd_fail(ctx, GGD_E_INVALID, "shs holds fewer coefficients than sh_degree needs");
  return GGD_OK;
}

// ---- forward ---------------------------------------------------------------------------------------------------
static const char* const kPendingMsg = "a frame enqueued with ggd_forward_enqueue is pending on this context: call ggd_forward_collect first";

// A frame begins (or, in the collection, ends): the context gets a fresh ggd_frame -- only the tag's sequence carries over -- and
// the caller the old one.
static ggd_frame frame_renew(ggd_ctx* ctx) {
  const ggd_frame old = ctx->frame;
  ctx->frame = ggd_frame();
  ctx->frame.r_tag = old.r_tag;
  return old;
}

// The folded front end's share of geometry_enqueue: workspace, the two alternating control blocks, this frame's plan.
static int fold_prepare(ggd_ctx* ctx, hipStream_t s, const ggd_params* prm, ggd_fold* fold) {
  const int nwg = (prm->P + 255) / 256;
  // [exclusive prefixes: nwg words | {sum, kept, ~min key, max key}: nwg uint4]
  int rc = grow_buffers(ctx, {{(void**)&ctx->scan_sums, sizeof(uint32_t)}}, &ctx->scan_sums_cap, 5 * (size_t)nwg + 64,
                        5 * (size_t)(nwg + nwg / 2) + 64);
  if (rc != GGD_OK) return rc;
  const size_t need = ggd_fold_block_words(prm->P);   // (status words and the instances per tile row behind them included)
  const bool fresh = ctx->foldctl_cap < need;   // (grow-only; both blocks start clean)
  rc = grow_buffers(ctx, {{(void**)&ctx->foldctl[0], sizeof(uint32_t)}, {(void**)&ctx->foldctl[1], sizeof(uint32_t)}},
                    &ctx->foldctl_cap, need, need + need / 2, &s);
  if (rc != GGD_OK) return rc;
  if (fresh) ctx->fold_cur = 0;
  if (fresh || ctx->fold_poisoned) {
    for (int b = 0; b < 2; ++b) {
      GGD_HIP(hipMemsetAsync(ctx->foldctl[b], 0, ctx->foldctl_cap * sizeof(uint32_t), s));
      ctx->foldctl_dirty[b] = 0;
    }
    ctx->fold_poisoned = false;
  }
  const int cur = ctx->fold_cur, oth = cur ^ 1;
  fold->ctl = ctx->foldctl[cur];
  fold->clear = ctx->foldctl[oth];
  fold->clear_words = (uint32_t)ctx->foldctl_dirty[oth];
  fold->wg_info = reinterpret_cast<uint4*>(ctx->scan_sums + (((size_t)nwg + 3) & ~(size_t)3));
  fold->rows = ((prm->width + 15) / 16 <= 64 && (prm->height + 15) / 16 <= 64) ? 1 : 0;
  fold->rowinst = ggd_fold_rowinst(fold->ctl, prm->P);
  // the two-launch depth sort is decided HERE because it selects the histograms this launch builds
  const ggd_spec_plan plan = ctx->spec.plan(ctx->opt[GGD_OPT_FOLD], ctx->opt[GGD_OPT_MSD_SORT], ggd_sort32_msd_supported(prm->P));
  fold->msd = plan.msd ? 1 : 0;
  fold->msd_lo = plan.lo; fold->msd_shift = plan.shift;
  ctx->foldctl_dirty[oth] = 0;       // (clean once this launch has run)
  ctx->foldctl_dirty[cur] = need;    // what this frame may write
  ctx->fold_cur = oth;
  ctx->frame.plan = plan;
  ctx->frame.geom.folded = true;
  return GGD_OK;
}

// Enqueue the per-Gaussian kernels + scan + the asynchronous read-back of {R, prefilter trap}; no host sync.
// (of `fb` the geometry buffer and radii; defer_scan: the scan is left to the depth sort of the render_enqueue that follows)
static int geometry_enqueue(ggd_ctx* ctx, void* stream, const ggd_params* prm, const ggd_inputs& in, const ggd_frame_bufs& fb,
                            int64_t* num_rendered, bool defer_scan) {
  (void)hipGetLastError();   // a sticky error another library left in this thread is not ours to report
  int rc = check_params(ctx, prm);
  if (rc != GGD_OK) return rc;
  rc = check_inputs(ctx, prm, in);
  if (rc != GGD_OK) return rc;
  if (!num_rendered) return ggd_fail(ctx, GGD_E_INVALID, "num_rendered is NULL");
  *num_rendered = 0;
  frame_renew(ctx);            // whatever an earlier frame left -- one that failed half way too -- ends here
  ggd_frame& fr = ctx->frame;
  if (prm->P == 0) return GGD_OK;
  if (!fb.geom_buf || !fb.radii || !in.opacities) return ggd_fail(ctx, GGD_E_INVALID, "geom_buf / radii / opacities is NULL");
  if (prm->raw_attributes && in.cov3D_precomp)
    return ggd_fail(ctx, GGD_E_INVALID, "raw_attributes needs scales/rotations (no cov3D_precomp)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const geom_ptrs g = geom_view(prm, fb.geom_buf);

  rc = ggd_reserve_scratch(ctx, ggd_scan_tmp_bytes(prm->P), s);
  if (rc != GGD_OK) return rc;
  if (prm->prefiltered) GGD_HIP(hipMemsetAsync(ctx->d_words + 1, 0, sizeof(uint32_t), s));
  // single-call forward on the tile-binning path: the scan (offsets + num_rendered) rides on the depth sort's launches, and the
  // sort's histograms + the scan's first step are produced by the preprocess kernel itself (ggd_fold)
  const bool ride = defer_scan && ctx->h_words_dev;
  ggd_fold fold;
  if (ride && ctx->opt[GGD_OPT_FOLD] != 0) {
    rc = fold_prepare(ctx, s, prm, &fold);
    if (rc != GGD_OK) return rc;
  }
  {
    StageTimer t(ctx, ST_PREPROCESS, s);
    const bool old_ctl = !fr.geom.folded && ctx->sortctl;
    rc = ggd_launch_preprocess(ctx, s, *prm, in, g.splat, g.tiles, in.shs ? g.clamped : nullptr, fb.radii, g.depth_keys, g.rect,
                               ctx->d_words + 1, old_ctl ? ctx->sortctl : nullptr, old_ctl ? (int)ggd_sort_ctrl_words() : 0,
                               fr.geom.folded ? &fold : nullptr);
    if (rc != GGD_OK) { ctx->fold_poisoned = fr.geom.folded; return rc; }
    fr.geom.sortctl_clean = old_ctl;
  }
  if (ride) {
    const size_t nb = (size_t)ggd_scan_blocks(prm->P);
    if (!fr.geom.folded) {
      rc = grow_buffers(ctx, {{(void**)&ctx->scan_sums, sizeof(uint32_t)}}, &ctx->scan_sums_cap, nb, nb + nb / 2 + 64);
      if (rc != GGD_OK) return rc;
    }
    if (prm->prefiltered)
      GGD_HIP(hipMemcpyAsync(ctx->h_words + 1, ctx->d_words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    fr.geom.ride = true;
    return GGD_OK;
  }
  {
    StageTimer t(ctx, ST_SCAN, s);
    rc = ggd_launch_inclusive_scan(ctx, s, g.tiles, g.offsets, prm->P, ctx->d_words, ctx->scratch, ctx->scratch_bytes,
                                   ctx->h_words_dev);
    if (rc != GGD_OK) return rc;
  }
  {
    StageTimer t(ctx, ST_READBACK, s);
    // with the device view of the pinned mirror the scan has already delivered R; only the prefilter trap word is copied
    if (!ctx->h_words_dev)
      GGD_HIP(hipMemcpyAsync(ctx->h_words, ctx->d_words, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    else if (prm->prefiltered)
      GGD_HIP(hipMemcpyAsync(ctx->h_words + 1, ctx->d_words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  return GGD_OK;
}

// Wait for the stream and publish R (the one host sync of a forward).
static int geometry_finish(ggd_ctx* ctx, void* stream, const ggd_params* prm, int64_t* num_rendered) {
  // The host needs num_rendered, not the finished frame: in the single-call forward it waits for the word written by the
  // launch that delivers R (early in the depth sort) and returns while binning and blend are still running -- as
  // upstream returns with its render kernels in flight.  Outputs are ordered on the caller's stream as usual.
  ggd_frame& fr = ctx->frame;
  if (fr.r_pending) {
    // the launch that carries the scan's block-sum step stores (tag << 32 | R) into the pinned mirror; poll for this
    // call's tag (an event record behind that launch would cost the GPU a ~6 us bubble between two kernels).  Every few
    // thousand polls the stream is queried: if it has drained without the tag (a failed launch), fall back to the copy.
    volatile unsigned long long* slot = reinterpret_cast<volatile unsigned long long*>(ctx->h_words + 2);
    const unsigned long long want = fr.r_tag;     // (30 bits; bit 63 of the word: this frame's top depth digit is constant,
                                                  // bit 62: the two-launch sort's histograms say it was valid for this frame)
    unsigned long long v = *slot;
    for (unsigned spins = 0; ((v >> 32) & 0x3fffffffull) != want; ++spins) {
      __builtin_ia32_pause();
      if ((spins & 0xfff) == 0xfff) {
        const hipError_t q = hipStreamQuery(static_cast<hipStream_t>(stream));
        if (q == hipSuccess) {
          v = *slot;
          if (((v >> 32) & 0x3fffffffull) != want) {   // fill the mirror as the launch would have
            uint32_t w6[6] = {0u, 0u, 0u, 0u, 0u, 0u};
            GGD_HIP(hipMemcpy(w6, ctx->d_words, sizeof(w6), hipMemcpyDeviceToHost));
            v = ((unsigned long long)(w6[2] & 1u) << 63) | ((unsigned long long)((w6[2] >> 1) & 1u) << 62) | (want << 32) | w6[0];
            ctx->h_words[4] = w6[3]; ctx->h_words[5] = w6[4]; ctx->h_words[6] = w6[5];
          }
          break;
        }
        if (q != hipErrorNotReady)   // the stream is in an error state: do not spin on a word that will never come
          return ggd_fail(ctx, GGD_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
      }
      v = *slot;
    }
    ctx->h_words[0] = (uint32_t)v;
    fr.report.flat = (v >> 63) != 0ull;
    fr.report.msd_ok = ((v >> 62) & 1ull) != 0ull;
    if (fr.report.folded) {   // only a folded frame's front end delivers the kept-key range: any other leaves the words as they were
      // (stored by the same device thread before the tagged word's release store; x86 loads are not reordered with earlier loads)
      volatile uint32_t* hw = ctx->h_words;
      fr.report.kmin = hw[4]; fr.report.kmax = hw[5]; fr.report.msd_flags = hw[6];
    }
  } else {
    GGD_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  }
  if (prm->prefiltered && ctx->h_words[1] != 0)
    return ggd_fail(ctx, GGD_E_PREFILTER, "Point is filtered although prefiltered is set. This shouldn't happen!");
  *num_rendered = (int64_t)ctx->h_words[0];
  return GGD_OK;
}

extern "C" int ggd_forward_geometry(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                                    const float* shs, const float* colors_precomp, const float* opacities,
                                    const float* scales, const float* rotations, const float* cov3D_precomp,
                                    void* geom_buf, int32_t* radii, int64_t* num_rendered) {
  if (ctx && ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_frame_bufs fb = {.geom_buf = geom_buf, .radii = radii};
  const int rc = geometry_enqueue(ctx, stream, prm, in, fb, num_rendered, false);
  if (rc != GGD_OK || prm->P == 0) return rc;
  return geometry_finish(ctx, stream, prm, num_rendered);
}

// The scratch of binning path 1: [four pair arrays | the depth sort's tmp, alive through the binning pass | the row binning's tmp | msd table]
struct sort_bin_scratch { uint32_t *ka, *va, *kb, *vb; void* sort_tmp; size_t sort_tmp_bytes; void* bin_tmp; size_t bin_tmp_bytes; uint32_t* msd_table; };
static int reserve_sort_bin_scratch(ggd_ctx* ctx, hipStream_t s, const ggd_params* prm, uint32_t capacity, bool msd,
                                    sort_bin_scratch* out) {
  const size_t pairs = ggd_align((size_t)prm->P * sizeof(uint32_t));
  out->sort_tmp_bytes = ggd_sort32_tmp_bytes(prm->P);
  out->bin_tmp_bytes = ggd_rowbin_tmp_bytes(prm->P, capacity, prm->width, prm->height);
  const size_t msd_tab = msd ? ggd_sort32_msd_table_bytes(prm->P) : 0;
  const int rc = ggd_reserve_scratch(ctx, 4 * pairs + out->sort_tmp_bytes + out->bin_tmp_bytes + msd_tab, s);
  if (rc != GGD_OK) return rc;
  char* next = static_cast<char*>(ctx->scratch);
  const auto take = [&next](size_t bytes) { uint32_t* p = reinterpret_cast<uint32_t*>(next); next += bytes; return p; };
  out->ka = take(pairs); out->va = take(pairs); out->kb = take(pairs); out->vb = take(pairs);
  out->sort_tmp = take(out->sort_tmp_bytes); out->bin_tmp = take(out->bin_tmp_bytes); out->msd_table = take(msd_tab);
  return GGD_OK;
}

// Binning path 1: depth-sort the Gaussians once (32-bit keys), then one stable row / column binning pass.  speculative: the true
// instance count is still on the device and `capacity` is only its upper bound (the launch geometry does not depend on it).
static int sort_depth_and_bin_tiles(ggd_ctx* ctx, hipStream_t s, const ggd_params* prm, const geom_ptrs& g, uint32_t* list,
                                    uint32_t* ranges, uint32_t capacity, bool speculative) {
  ggd_frame& fr = ctx->frame;
  const bool riding = fr.geom.ride;                  // this call's geometry half left the scan to us
  const bool folded = riding && fr.geom.folded;      // ... and its preprocess filled the histograms
  const bool msd = folded && fr.plan.msd;            // ... those of the two-launch sort
  // the control block this frame's preprocess cleared, if nobody has used it since (a second render of the same geometry
  // falls back to the memset)
  uint32_t* clean_ctl = fr.geom.sortctl_clean ? ctx->sortctl : nullptr;
  fr.geom = {};
  sort_bin_scratch w;
  int rc = reserve_sort_bin_scratch(ctx, s, prm, capacity, msd, &w);
  if (rc != GGD_OK) return rc;
  ggd_scan_piggy pg;          // a scan that rides on this call's launches (see geometry_enqueue)
  ggd_fold fold;              // the folded front end's control block, if this call has one
  const uint32_t *n_vis_ptr = nullptr, *flat_ptr = nullptr;   // device words: kept keys, "last pass was flat"
  const bool narrow = !rb_is_wide(prm->width, prm->height);   // grids of <= 64 x 64 tiles: the lane-per-bin binning kernels
  bool counted = false;                                       // this frame's level 1 takes its row counts from the sort's finish launch
  {
    StageTimer t(ctx, ST_SORT, s);
    if (riding) {
      pg.in = g.tiles; pg.out = g.offsets;
      pg.n = prm->P; pg.nb = ggd_scan_blocks(prm->P); pg.block_sums = ctx->scan_sums;
      pg.d_total = ctx->d_words; pg.h_total = ctx->h_words_dev;
      pg.h_tagged = reinterpret_cast<unsigned long long*>(ctx->h_words_dev + 2);
      pg.tag = fr.r_tag = fr.r_tag % 0x3fffffffu + 1u;   // 1 .. 2^30 - 1 in turn
      if (folded) {
        const int nwg = (prm->P + 255) / 256;
        fold.ctl = ctx->foldctl[ctx->fold_cur ^ 1];   // (fold_cur already points at the next frame's block)
        pg.wg_info = reinterpret_cast<const uint4*>(ctx->scan_sums + (((size_t)nwg + 3) & ~(size_t)3));
        pg.n_info = nwg;
        pg.sum_stride = 8;                            // 2048-element scan blocks over 256-point workgroup prefixes
      }
    }
    if (msd && !speculative) return ggd_fail(ctx, GGD_E_INVALID, "internal: two-launch sort outside the speculative tile-binning path");
    // the fourth pass is an empty launch when the depths' top byte is constant: after GGD_FLAT_STREAK such frames it is not
    // launched; the collection re-renders a frame for which that was wrong (report.flat arrives with num_rendered)
    fr.three_passes = ctx->spec.three_passes(fr.plan, folded, speculative, ctx->opt[GGD_OPT_FOLD]);
    fr.report.folded = folded;
    fold.msd = msd ? 1 : 0;
    fold.msd_lo = fr.plan.lo; fold.msd_shift = fr.plan.shift;
    if (msd) {
      // counted level 1: the finish launch also fills the row tables in the binning's scratch (narrow grids; GGD_OPT_L1_COUNTED)
      counted = ctx->opt[GGD_OPT_L1_COUNTED] != 0 && narrow;
      const ggd_l1_counted l1c = ggd_rowbin_counted(w.bin_tmp, g.rect, prm->P, capacity, prm->width, prm->height);
      rc = ggd_launch_sort32_msd(ctx, s, g.depth_keys, w.ka, w.va, w.kb, w.vb, prm->P, w.msd_table, &pg, &fold,
                                 counted ? &l1c : nullptr);
    } else {
      ggd_sort32_opts so;
      so.clean_ctl = folded ? nullptr : clean_ctl;
      so.piggy = riding ? &pg : nullptr;
      so.fold = folded ? &fold : nullptr;
      so.flag_flat_last = true;
      so.apply_here = false;             // the offsets are left to the binning's last launch
      so.skip_last = fr.three_passes;
      rc = ggd_launch_sort32_iota(ctx, s, g.depth_keys, w.ka, w.va, w.kb, w.vb, prm->P, 32, w.sort_tmp, w.sort_tmp_bytes, so);
    }
    if (rc != GGD_OK) return rc;
    fr.r_pending = riding;
    const ggd_sort_ctl sc = ggd_sort_ctl::select(w.sort_tmp, clean_ctl, folded ? fold.ctl : nullptr);
    n_vis_ptr = sc.n_valid; flat_ptr = sc.flat;
  }
  StageTimer t(ctx, ST_DUPLICATE, s);
  // the depth sort dropped the culled Gaussians (key 0xFFFFFFFF) and left the number of kept ones on the device
  ggd_rowbin_opts ro = {.order_alt = w.vb, .use_alt = flat_ptr, .apply = riding ? &pg : nullptr};
  if (folded && narrow)   // level 1 in one launch
    ro.fold = {.rowtot = ggd_fold_rowtot(fold.ctl), .status1 = ggd_fold_l1_status(fold.ctl, prm->P),
               .rowinst = ggd_fold_rowinst(fold.ctl, prm->P)};
  if (counted) ro.counted_hist = ggd_sort_ctl::in_fold(fold.ctl).ghist;
  const ggd_rowbin_result rb = ggd_launch_rowbin(ctx, s, *prm, g.rect, w.va, n_vis_ptr, list, ranges, capacity, w.bin_tmp,
                                                 w.bin_tmp_bytes, ro);
  if (rb.scan_in_scatter) ++ctx->scan_in_scatter_frames;
  if (counted && rb.rc == GGD_OK) ++ctx->l1_counted_frames;
  return rb.rc;
}

// Binning path 2 (GGD_OPT_BINNING = 0, the debug taps, grids beyond 255 x 255 tiles, R = 0): one (tile | depth) key per instance,
// a 64-bit sort, tile ranges by boundary detection.
static int duplicate_sort_ranges(ggd_ctx* ctx, hipStream_t s, const ggd_params* prm, const geom_ptrs& g, const binning_ptrs& b,
                                 uint32_t* ranges, int64_t R) {
  const int T = ((prm->width + 15) / 16) * ((prm->height + 15) / 16);
  int rc = GGD_OK;
  if (R > 0) {
    const int nbits = ggd_sort_bits(prm->width, prm->height);
    const size_t sort_tmp = ggd_sort_tmp_bytes(R);
    rc = ggd_reserve_scratch(ctx, sort_tmp, s);
    if (rc != GGD_OK) return rc;
    const bool to_alt = ggd_sort_input_is_alt(nbits) != 0;
    uint64_t* k0 = to_alt ? b.keys_alt : b.keys;
    uint32_t* v0 = to_alt ? b.list_alt : b.list;
    {
      StageTimer t(ctx, ST_DUPLICATE, s);
      rc = ggd_launch_duplicate(ctx, s, *prm, g.rect, g.depth_keys, g.tiles, g.offsets, k0, v0);
      if (rc != GGD_OK) return rc;
    }
    if (prm->debug) {
      rc = grow_buffers(ctx, {{&ctx->dbg_keys, sizeof(uint64_t)}, {&ctx->dbg_vals, sizeof(uint32_t)}}, &ctx->dbg_cap, (size_t)R, (size_t)R);
      if (rc != GGD_OK) return rc;
      GGD_HIP(hipMemcpyAsync(ctx->dbg_keys, k0, (size_t)R * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
      GGD_HIP(hipMemcpyAsync(ctx->dbg_vals, v0, (size_t)R * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    }
    StageTimer t(ctx, ST_SORT, s);
    rc = ggd_launch_sort(ctx, s, b.keys, b.list, b.keys_alt, b.list_alt, R, nbits, ctx->scratch, ctx->scratch_bytes);
    if (rc != GGD_OK) return rc;
  }
  StageTimer t(ctx, ST_RANGES, s);
  return ggd_launch_ranges(ctx, s, b.keys, R, ranges, T);
}

// the kernels bound their list positions with a 32-bit R
static uint32_t list_capacity(int64_t R) { return R > 0xffffffffll ? 0xffffffffu : (uint32_t)R; }

// R: number of instances to process (<= fb.capacity; equal unless the caller over-allocated).  speculative: R is only a CAPACITY
// (the true num_rendered is still on the device); only the tile-binning path can run that way
static int render_enqueue(ggd_ctx* ctx, void* stream, const ggd_params* prm, const ggd_frame_bufs& fb, int64_t R,
                          bool speculative) {
  (void)hipGetLastError();   // a sticky error another library left in this thread is not ours to report
  int rc = check_params(ctx, prm);
  if (rc != GGD_OK) return rc;
  if (R < 0) return ggd_fail(ctx, GGD_E_INVALID, "num_rendered < 0");
  if (!fb.img_buf || !fb.out_color) return ggd_fail(ctx, GGD_E_INVALID, "img_buf / out_color is NULL");
  if (R > 0 && (!fb.geom_buf || !fb.binning_buf)) return ggd_fail(ctx, GGD_E_INVALID, "geom_buf / binning_buf is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const geom_ptrs g = geom_view(prm, fb.geom_buf);
  const binning_ptrs b = binning_view(fb.capacity, fb.binning_buf);
  const img_ptrs im = img_view(prm->width, prm->height, fb.img_buf);
  const bool tiles = use_tile_binning(ctx, prm, R);
  if (speculative && !tiles) return ggd_fail(ctx, GGD_E_INVALID, "speculative render needs the tile-binning path");
  const uint32_t capacity = list_capacity(R);
  rc = (R > 0 && tiles) ? sort_depth_and_bin_tiles(ctx, s, prm, g, b.list, im.ranges, capacity, speculative)
                        : duplicate_sort_ranges(ctx, s, prm, g, b, im.ranges, R);
  if (rc != GGD_OK) return rc;
  StageTimer t(ctx, ST_BLEND, s);
  return ggd_launch_blend(ctx, s, *prm, g.splat, b.list, im.ranges, capacity, fb.out_color, im.final_T, im.n_contrib, g.depth_keys,
                          fb.out_depth, fb.out_alpha);
}

extern "C" int ggd_forward_render(ggd_ctx* ctx, void* stream, const ggd_params* prm, const void* geom_buf,
                                  int64_t R, void* binning_buf, void* img_buf, float* out_color) {
  // (another forward would begin a new ctx->frame: the pending one's missed speculation would never be rendered again)
  if (ctx && ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  const ggd_frame_bufs fb = {.geom_buf = const_cast<void*>(geom_buf), .binning_buf = binning_buf, .capacity = R,   // (laid out for R)
                             .img_buf = img_buf, .out_color = out_color};
  return render_enqueue(ctx, stream, prm, fb, R, false);
}

static int check_aux_planes(ggd_ctx* ctx, const float* out_depth, const float* out_alpha) {
  if (!ctx) return GGD_E_INVALID;
  if (!out_depth || !out_alpha) return ggd_fail(ctx, GGD_E_INVALID, "out_depth / out_alpha is NULL");
  return GGD_OK;
}

extern "C" int ggd_forward_render_aux(ggd_ctx* ctx, void* stream, const ggd_params* prm, const void* geom_buf,
                                      int64_t R, void* binning_buf, void* img_buf, float* out_color, float* out_depth,
                                      float* out_alpha) {
  const int rc = check_aux_planes(ctx, out_depth, out_alpha);
  if (rc != GGD_OK) return rc;
  if (ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  const ggd_frame_bufs fb = {.geom_buf = const_cast<void*>(geom_buf), .binning_buf = binning_buf, .capacity = R,
                             .img_buf = img_buf, .out_color = out_color, .out_depth = out_depth, .out_alpha = out_alpha};
  return render_enqueue(ctx, stream, prm, fb, R, false);
}

extern "C" int ggd_forward_can_speculate(ggd_ctx* ctx, const ggd_params* prm, int64_t capacity) {
  return ctx && prm && prm->P > 0 && use_tile_binning(ctx, prm, capacity) ? 1 : 0;
}

// The speculative route of the single-call forward in its two halves: everything is enqueued before the host looks at
// num_rendered (the GPU never idles on that read-back) ...
static int forward_spec_enqueue(ggd_ctx* ctx, void* stream, const ggd_params* prm, const ggd_inputs& in, const ggd_frame_bufs& fb,
                                int64_t* num_rendered) {
  const int rc = geometry_enqueue(ctx, stream, prm, in, fb, num_rendered, true);
  if (rc != GGD_OK) return rc;
  return render_enqueue(ctx, stream, prm, fb, fb.capacity, true);
}
// ... and the collection of num_rendered and the frame's report once the launch that delivers them has run; binning and blend
// may still be running.  A frame for which the short form of the sort did not hold is binned and blended again, in full.
static int forward_spec_collect(ggd_ctx* ctx, void* stream, const ggd_params* prm, const ggd_frame_bufs& fb,
                                int64_t* num_rendered) {
  const int rc = geometry_finish(ctx, stream, prm, num_rendered);
  if (rc != GGD_OK) return rc;
  const ggd_frame done = frame_renew(ctx);   // (a re-render below is a frame of its own: nothing to ride on, nothing to collect)
  const bool too_small = *num_rendered > fb.capacity;
  const bool again = ctx->spec.observe(done.plan, done.three_passes, done.report, too_small);
  if (too_small)
    return ggd_fail(ctx, GGD_E_CAPACITY, "binning_buf capacity is below num_rendered: re-run with a larger buffer");
  if (!again) return GGD_OK;
  return render_enqueue(ctx, stream, prm, fb, *num_rendered, false);
}

static int forward_single_call(ggd_ctx* ctx, void* stream, const ggd_params* prm, const ggd_inputs& in, const ggd_frame_bufs& fb,
                               int64_t* num_rendered) {
  if (fb.capacity < 0) return ggd_fail(ctx, GGD_E_INVALID, "capacity < 0");
  if (ctx && ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  if (prm && prm->P > 0 && fb.capacity > 0 && ggd_forward_can_speculate(ctx, prm, fb.capacity)) {
    const int rc = forward_spec_enqueue(ctx, stream, prm, in, fb, num_rendered);
    if (rc != GGD_OK) return rc;
    return forward_spec_collect(ctx, stream, prm, fb, num_rendered);
  }
  int rc = geometry_enqueue(ctx, stream, prm, in, fb, num_rendered, false);
  if (rc != GGD_OK) return rc;
  if (prm->P == 0) return render_enqueue(ctx, stream, prm, fb, 0, false);
  rc = geometry_finish(ctx, stream, prm, num_rendered);
  if (rc != GGD_OK) return rc;
  if (*num_rendered > fb.capacity)
    return ggd_fail(ctx, GGD_E_CAPACITY, "binning_buf capacity is below num_rendered: re-run with a larger buffer");
  return render_enqueue(ctx, stream, prm, fb, *num_rendered, false);
}

extern "C" int ggd_forward(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D, const float* shs,
                           const float* colors_precomp, const float* opacities, const float* scales,
                           const float* rotations, const float* cov3D_precomp, void* geom_buf, int32_t* radii,
                           void* binning_buf, int64_t capacity, void* img_buf, float* out_color,
                           int64_t* num_rendered) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_frame_bufs fb = {.geom_buf = geom_buf, .radii = radii, .binning_buf = binning_buf, .capacity = capacity,
                             .img_buf = img_buf, .out_color = out_color};
  return forward_single_call(ctx, stream, prm, in, fb, num_rendered);
}

extern "C" int ggd_forward_aux(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D, const float* shs,
                               const float* colors_precomp, const float* opacities, const float* scales,
                               const float* rotations, const float* cov3D_precomp, void* geom_buf, int32_t* radii,
                               void* binning_buf, int64_t capacity, void* img_buf, float* out_color, float* out_depth,
                               float* out_alpha, int64_t* num_rendered) {
  const int rc = check_aux_planes(ctx, out_depth, out_alpha);
  if (rc != GGD_OK) return rc;
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_frame_bufs fb = {.geom_buf = geom_buf, .radii = radii, .binning_buf = binning_buf, .capacity = capacity,
                             .img_buf = img_buf, .out_color = out_color, .out_depth = out_depth, .out_alpha = out_alpha};
  return forward_single_call(ctx, stream, prm, in, fb, num_rendered);
}

extern "C" int ggd_forward_enqueue(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D, const float* shs,
                                   const float* colors_precomp, const float* opacities, const float* scales,
                                   const float* rotations, const float* cov3D_precomp, void* geom_buf, int32_t* radii,
                                   void* binning_buf, int64_t capacity, void* img_buf, float* out_color) {
  if (!ctx) return GGD_E_INVALID;
  if (ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_enqueue: the previous frame of this context has not been collected");
  if (!prm || prm->P <= 0 || capacity <= 0 || !ggd_forward_can_speculate(ctx, prm, capacity))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_enqueue needs the tile-binning path, P > 0 and a capacity (ggd_forward_can_speculate)");
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_frame_bufs fb = {.geom_buf = geom_buf, .radii = radii, .binning_buf = binning_buf, .capacity = capacity,
                             .img_buf = img_buf, .out_color = out_color};
  int64_t dummy = 0;
  const int rc = forward_spec_enqueue(ctx, stream, prm, in, fb, &dummy);
  if (rc != GGD_OK) return rc;
  ctx->pending = {true, *prm, fb};
  return GGD_OK;
}

extern "C" int ggd_forward_collect(ggd_ctx* ctx, void* stream, int64_t* num_rendered) {
  if (!ctx || !num_rendered) return GGD_E_INVALID;
  if (!ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_collect: no frame is pending on this context");
  ctx->pending.valid = false;
  return forward_spec_collect(ctx, stream, &ctx->pending.prm, ctx->pending.bufs, num_rendered);
}

// ---- backward --------------------------------------------------------------------------------------------------
// entry: which entry point called.  ggd_backward_aux always runs the depth / alpha (AUX) instances, with both of its gradients NULL
// too; ggd_backward_abs the absgrad ones, with the depth / alpha terms exactly when one of the two gradients is given (without: the
// plain backward's arithmetic).  radii and the three buffers are the forward's, R its num_rendered
// feat (ggd_backward_features): the feature blend's backward runs between the blend backward and the per-Gaussian backward and
// adds to the same accumulator records; the depth / alpha terms run exactly when one of their gradients is given
// dL_ddist (ggd_backward_distortion): the distortion map's backward runs in the same place; always with the AUX instances, whose
// per-Gaussian kernel turns the accumulator's z slot into dL_dmeans3D.  It may carry a feature map as well (feat)
// cam (ggd_backward_camera): the camera's gradients, two more launches behind the per-Gaussian backward on the same accumulator
// records.  In front of them the call is the one its other arguments describe: dL_ddist as ggd_backward_distortion, else feat as
// ggd_backward_features, else ggd_backward_aux with a depth or alpha gradient and ggd_backward without
enum bwd_entry { BWD_PLAIN, BWD_AUX, BWD_ABS, BWD_FEATURES, BWD_DISTORTION, BWD_CAMERA };
struct bwd_features {     // the feature map's side of ggd_backward_features
  const float* features = nullptr; int C = 0; const float* feature_bg = nullptr;
  const float* dL_dfeatmap = nullptr; float* dL_dfeatures = nullptr;
};
// the C ABI's bundle as backward_impl takes it, in `store`; NULL (no feature map) stays NULL
static const bwd_features* feature_side(const ggd_feature_side* f, bwd_features& store) {
  if (!f) return nullptr;
  store = {.features = f->features, .C = f->C, .feature_bg = f->feature_bg, .dL_dfeatmap = f->dL_dfeatmap, .dL_dfeatures = f->dL_dfeatures};
  return &store;
}
static int check_feature_channels(ggd_ctx* ctx, int C) {
  if (C < 1 || C > GGD_FEATURES_MAX_CHANNELS)
    return ggd_fail(ctx, GGD_E_INVALID, "feature channels C = " + std::to_string(C) + " outside 1 .. " + std::to_string(GGD_FEATURES_MAX_CHANNELS));
  return GGD_OK;
}
static int backward_impl(ggd_ctx* ctx, void* stream, const ggd_params* prm, bwd_entry entry, const ggd_inputs& in,
                         const int32_t* radii, const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                         const ggd_pix_grads& pix, const ggd_grads& out, const bwd_features* feat = nullptr,
                         const float* dL_ddist = nullptr, const ggd_camera_grads* cam = nullptr) {
  (void)hipGetLastError();   // a sticky error another library left in this thread is not ours to report
  int rc = check_params(ctx, prm);
  if (rc != GGD_OK) return rc;
  rc = check_inputs(ctx, prm, in);
  if (rc != GGD_OK) return rc;
  const int P = prm->P;
  if (feat) {
    rc = check_feature_channels(ctx, feat->C);
    if (rc != GGD_OK) return rc;
    if (P > 0 && (!feat->features || !feat->dL_dfeatmap || !feat->dL_dfeatures))
      return ggd_fail(ctx, GGD_E_INVALID, "ggd_backward_features: features / dL_dfeatmap / dL_dfeatures is NULL");
  }
  if (entry == BWD_DISTORTION && !dL_ddist) return ggd_fail(ctx, GGD_E_INVALID, "ggd_backward_distortion: dL_ddistortion is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (entry == BWD_CAMERA) {
    if (!cam || !cam->dL_dviewmatrix || !cam->dL_dprojmatrix || !cam->dL_dcampos)
      return ggd_fail(ctx, GGD_E_INVALID, "ggd_backward_camera: the camera bundle or one of its members is NULL");
    if (P == 0 || R <= 0) {   // nothing was blended: every accumulator record is zero, and so are the sums
      GGD_HIP(hipMemsetAsync(cam->dL_dviewmatrix, 0, 16 * sizeof(float), s));
      GGD_HIP(hipMemsetAsync(cam->dL_dprojmatrix, 0, 16 * sizeof(float), s));
      GGD_HIP(hipMemsetAsync(cam->dL_dcampos, 0, 3 * sizeof(float), s));
    }
  }
  if (P == 0) return GGD_OK;
  if (!radii || !geom_buf || !img_buf || !pix.dL_dpix || !out.dL_dmeans2D || !out.dL_dcolors || !out.dL_dopacity ||
      !out.dL_dmeans3D || !out.dL_dcov3D || !out.dL_dscales || !out.dL_drots || (prm->M > 0 && !out.dL_dsh) ||
      (R > 0 && !binning_buf))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_backward: NULL buffer");
  const bool abs = entry == BWD_ABS;
  const bool aux = entry == BWD_AUX || entry == BWD_DISTORTION || dL_ddist ||
                   ((abs || entry == BWD_FEATURES || entry == BWD_CAMERA) && (pix.dL_ddepth || pix.dL_dalpha));
  if (abs && !out.dL_dmeans2D_abs) return ggd_fail(ctx, GGD_E_INVALID, "ggd_backward_abs: NULL dL_dmeans2D_abs");
  if (prm->raw_attributes && (!in.opacities || in.cov3D_precomp))
    return ggd_fail(ctx, GGD_E_INVALID, "raw_attributes needs opacities and scales/rotations (no cov3D_precomp)");
  if (prm->antialiasing && !in.opacities)   // dL/dh of the opacity compensation is dL/do_eff times the opacity
    return ggd_fail(ctx, GGD_E_INVALID, "antialiasing needs the opacities in the backward");
  const geom_ptrs g = geom_view(prm, geom_buf);
  const binning_ptrs b = binning_view(R, binning_buf);
  const img_ptrs im = img_view(prm->width, prm->height, img_buf);

  const size_t acc_bytes = (size_t)P * GGD_ACC_FLOATS * sizeof(float);
  const bool cam_sums = entry == BWD_CAMERA && R > 0;   // (their partial rows lie behind the accumulator records)
  rc = ggd_reserve_scratch(ctx, ggd_align(acc_bytes) + (cam_sums ? ggd_align(ggd_camera_tmp_bytes(P)) : 0), s);
  if (rc != GGD_OK) return rc;
  float* grad_acc = static_cast<float*>(ctx->scratch);
  // the only zero-fill of the backward: the accumulator records.  Every caller array is written in full by the
  // per-Gaussian kernel, except the ones a mode never produces (kept zero like upstream's zero-initialised outputs).
  GGD_HIP(hipMemsetAsync(grad_acc, 0, acc_bytes, s));
  if (in.cov3D_precomp) {
    GGD_HIP(hipMemsetAsync(out.dL_dscales, 0, (size_t)P * 3 * sizeof(float), s));
    GGD_HIP(hipMemsetAsync(out.dL_drots, 0, (size_t)P * 4 * sizeof(float), s));
  }
  if (in.colors_precomp && prm->M > 0 && out.dL_dsh)
    GGD_HIP(hipMemsetAsync(out.dL_dsh, 0, (size_t)P * prm->M * 3 * sizeof(float), s));
  if (feat) GGD_HIP(hipMemsetAsync(feat->dL_dfeatures, 0, (size_t)P * feat->C * sizeof(float), s));

  if (R > 0) {
    StageTimer t(ctx, ST_BLEND_BWD, s);
    rc = ggd_launch_blend_backward(ctx, s, *prm, g.splat, b.list, im.ranges, im.final_T, im.n_contrib, pix, grad_acc, aux,
                                   g.depth_keys, abs);
    if (rc != GGD_OK) return rc;
    if (feat) {
      rc = ggd_launch_features_backward(ctx, s, *prm, g.splat, b.list, im.ranges, list_capacity(R),
                                        im.final_T, im.n_contrib, feat->features, feat->C, feat->feature_bg, feat->dL_dfeatmap,
                                        grad_acc, feat->dL_dfeatures);
      if (rc != GGD_OK) return rc;
    }
    if (dL_ddist) {
      rc = ggd_launch_distortion_backward(ctx, s, *prm, g.splat, b.list, im.ranges, list_capacity(R),
                                          im.final_T, im.n_contrib, g.depth_keys, dL_ddist, grad_acc);
      if (rc != GGD_OK) return rc;
    }
  }
  {
    StageTimer t(ctx, ST_PREPROCESS_BWD, s);
    rc = ggd_launch_preprocess_backward(ctx, s, *prm, in, radii, in.shs ? g.clamped : nullptr, grad_acc, out, aux);
    if (rc != GGD_OK) return rc;
  }
  if (cam_sums) {
    float* partial = reinterpret_cast<float*>(static_cast<char*>(ctx->scratch) + ggd_align(acc_bytes));
    rc = ggd_launch_camera_backward(ctx, s, *prm, in, radii, in.shs ? g.clamped : nullptr, grad_acc, aux, partial, *cam);
    if (rc != GGD_OK) return rc;
  }
  return GGD_OK;
}

extern "C" int ggd_backward(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                            const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                            const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                            const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                            const float* dL_dpix, float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                            float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                            float* dL_drots) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_pix_grads pix = {.dL_dpix = dL_dpix};
  const ggd_grads out = {.dL_dmeans2D = dL_dmeans2D, .dL_dcolors = dL_dcolors, .dL_dopacity = dL_dopacity,
                         .dL_dmeans3D = dL_dmeans3D, .dL_dcov3D = dL_dcov3D, .dL_dsh = dL_dsh, .dL_dscales = dL_dscales,
                         .dL_drots = dL_drots};
  return backward_impl(ctx, stream, prm, BWD_PLAIN, in, radii, geom_buf, binning_buf, img_buf, R, pix, out);
}

extern "C" int ggd_backward_aux(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                                const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                                const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                                const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans2D,
                                float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                float* dL_dscales, float* dL_drots) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_pix_grads pix = {.dL_dpix = dL_dpix, .dL_ddepth = dL_ddepth, .dL_dalpha = dL_dalpha};
  const ggd_grads out = {.dL_dmeans2D = dL_dmeans2D, .dL_dcolors = dL_dcolors, .dL_dopacity = dL_dopacity,
                         .dL_dmeans3D = dL_dmeans3D, .dL_dcov3D = dL_dcov3D, .dL_dsh = dL_dsh, .dL_dscales = dL_dscales,
                         .dL_drots = dL_drots};
  return backward_impl(ctx, stream, prm, BWD_AUX, in, radii, geom_buf, binning_buf, img_buf, R, pix, out);
}

// the absgrad backward: ggd_backward_aux's arguments + dL_dmeans2D_abs
extern "C" int ggd_backward_abs(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                                const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                                const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                                const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans2D,
                                float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                float* dL_dscales, float* dL_drots, float* dL_dmeans2D_abs) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_pix_grads pix = {.dL_dpix = dL_dpix, .dL_ddepth = dL_ddepth, .dL_dalpha = dL_dalpha};
  const ggd_grads out = {.dL_dmeans2D = dL_dmeans2D, .dL_dcolors = dL_dcolors, .dL_dopacity = dL_dopacity,
                         .dL_dmeans3D = dL_dmeans3D, .dL_dcov3D = dL_dcov3D, .dL_dsh = dL_dsh, .dL_dscales = dL_dscales,
                         .dL_drots = dL_drots, .dL_dmeans2D_abs = dL_dmeans2D_abs};
  return backward_impl(ctx, stream, prm, BWD_ABS, in, radii, geom_buf, binning_buf, img_buf, R, pix, out);
}

// the feature maps: ggd_forward_features after a completed forward; ggd_backward_features = ggd_backward_aux's arguments + the
// feature side
extern "C" int ggd_forward_features(ggd_ctx* ctx, void* stream, const ggd_params* prm, const void* geom_buf,
                                    const void* binning_buf, const void* img_buf, int64_t R, const float* features, int32_t C,
                                    const float* feature_bg, float* out_features) {
  if (!ctx) return GGD_E_INVALID;
  (void)hipGetLastError();
  int rc = check_params(ctx, prm);
  if (rc != GGD_OK) return rc;
  rc = check_feature_channels(ctx, C);
  if (rc != GGD_OK) return rc;
  if (ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  if (R < 0) return ggd_fail(ctx, GGD_E_INVALID, "num_rendered < 0");
  if (!out_features || !img_buf) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_features: img_buf / out_features is NULL");
  if (prm->P > 0 && !features) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_features: features is NULL");
  if (R > 0 && (!geom_buf || !binning_buf)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_features: geom_buf / binning_buf is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const geom_ptrs g = geom_view(prm, geom_buf);
  const binning_ptrs b = binning_view(R, binning_buf);
  const img_ptrs im = img_view(prm->width, prm->height, img_buf);
  return ggd_launch_features_forward(ctx, s, *prm, g.splat, b.list, im.ranges, list_capacity(R),
                                     im.n_contrib, features, C, feature_bg, out_features);
}

extern "C" int ggd_backward_features(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                                     const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                                     const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                     const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                                     const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, const float* features,
                                     int32_t C, const float* feature_bg, const float* dL_dfeatmap, float* dL_dmeans2D,
                                     float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                     float* dL_dscales, float* dL_drots, float* dL_dfeatures) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_pix_grads pix = {.dL_dpix = dL_dpix, .dL_ddepth = dL_ddepth, .dL_dalpha = dL_dalpha};
  const ggd_grads out = {.dL_dmeans2D = dL_dmeans2D, .dL_dcolors = dL_dcolors, .dL_dopacity = dL_dopacity,
                         .dL_dmeans3D = dL_dmeans3D, .dL_dcov3D = dL_dcov3D, .dL_dsh = dL_dsh, .dL_dscales = dL_dscales,
                         .dL_drots = dL_drots};
  const bwd_features feat = {.features = features, .C = C, .feature_bg = feature_bg, .dL_dfeatmap = dL_dfeatmap,
                             .dL_dfeatures = dL_dfeatures};
  return backward_impl(ctx, stream, prm, BWD_FEATURES, in, radii, geom_buf, binning_buf, img_buf, R, pix, out, &feat);
}

// the distortion map: ggd_forward_distortion after a completed forward; ggd_backward_distortion = ggd_backward_aux's arguments +
// dL_ddistortion and, optionally, the feature map's side of ggd_backward_features as one bundle
extern "C" int ggd_forward_distortion(ggd_ctx* ctx, void* stream, const ggd_params* prm, const void* geom_buf,
                                      const void* binning_buf, const void* img_buf, int64_t R, float* out_distortion) {
  if (!ctx) return GGD_E_INVALID;
  (void)hipGetLastError();
  const int rc = check_params(ctx, prm);
  if (rc != GGD_OK) return rc;
  if (ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  if (R < 0) return ggd_fail(ctx, GGD_E_INVALID, "num_rendered < 0");
  if (!out_distortion || !img_buf) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_distortion: img_buf / out_distortion is NULL");
  if (R > 0 && (!geom_buf || !binning_buf)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_forward_distortion: geom_buf / binning_buf is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const geom_ptrs g = geom_view(prm, geom_buf);
  const binning_ptrs b = binning_view(R, binning_buf);
  const img_ptrs im = img_view(prm->width, prm->height, img_buf);
  return ggd_launch_distortion_forward(ctx, s, *prm, g.splat, b.list, im.ranges, list_capacity(R),
                                       im.n_contrib, g.depth_keys, out_distortion);
}

// the contribution statistics: ggd_contribution after a completed forward, accumulated into stats [P][3]
extern "C" int ggd_contribution(ggd_ctx* ctx, void* stream, const ggd_params* prm, const void* geom_buf,
                                const void* binning_buf, const void* img_buf, int64_t R, int64_t* stats) {
  if (!ctx) return GGD_E_INVALID;
  (void)hipGetLastError();
  const int rc = check_params(ctx, prm);
  if (rc != GGD_OK) return rc;
  if (ctx->pending.valid) return ggd_fail(ctx, GGD_E_INVALID, kPendingMsg);
  if (R < 0) return ggd_fail(ctx, GGD_E_INVALID, "num_rendered < 0");
  if (prm->P > 0 && !stats) return ggd_fail(ctx, GGD_E_INVALID, "ggd_contribution: stats is NULL");
  if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_contribution: stats is not 8-byte aligned");
  if (!img_buf) return ggd_fail(ctx, GGD_E_INVALID, "ggd_contribution: img_buf is NULL");
  if (R > 0 && (!geom_buf || !binning_buf)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_contribution: geom_buf / binning_buf is NULL");
  if (prm->P == 0 || R == 0) return GGD_OK;   // no pair: nothing to add
  hipStream_t s = static_cast<hipStream_t>(stream);
  const geom_ptrs g = geom_view(prm, geom_buf);
  const binning_ptrs b = binning_view(R, binning_buf);
  const img_ptrs im = img_view(prm->width, prm->height, img_buf);
  return ggd_launch_contribution(ctx, s, *prm, g.splat, b.list, im.ranges, list_capacity(R), im.n_contrib, stats);
}

extern "C" int ggd_backward_distortion(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                                       const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                                       const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                       const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                                       const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans2D,
                                       float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                       float* dL_dscales, float* dL_drots, const float* dL_ddistortion,
                                       const ggd_feature_side* features) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_pix_grads pix = {.dL_dpix = dL_dpix, .dL_ddepth = dL_ddepth, .dL_dalpha = dL_dalpha};
  const ggd_grads out = {.dL_dmeans2D = dL_dmeans2D, .dL_dcolors = dL_dcolors, .dL_dopacity = dL_dopacity,
                         .dL_dmeans3D = dL_dmeans3D, .dL_dcov3D = dL_dcov3D, .dL_dsh = dL_dsh, .dL_dscales = dL_dscales,
                         .dL_drots = dL_drots};
  bwd_features feat;
  return backward_impl(ctx, stream, prm, BWD_DISTORTION, in, radii, geom_buf, binning_buf, img_buf, R, pix, out, feature_side(features, feat),
                       dL_ddistortion);
}

// the camera's gradients: ggd_backward_distortion's arguments, each map's side optional, + the bundle of the three results
extern "C" int ggd_backward_camera(ggd_ctx* ctx, void* stream, const ggd_params* prm, const float* means3D,
                                   const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                                   const float* rotations, const float* cov3D_precomp, const int32_t* radii,
                                   const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t R,
                                   const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans2D,
                                   float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                   float* dL_dscales, float* dL_drots, const float* dL_ddistortion,
                                   const ggd_feature_side* features, const ggd_camera_grads* camera) {
  const ggd_inputs in = {.means3D = means3D, .shs = shs, .colors_precomp = colors_precomp, .opacities = opacities,
                         .scales = scales, .rotations = rotations, .cov3D_precomp = cov3D_precomp};
  const ggd_pix_grads pix = {.dL_dpix = dL_dpix, .dL_ddepth = dL_ddepth, .dL_dalpha = dL_dalpha};
  const ggd_grads out = {.dL_dmeans2D = dL_dmeans2D, .dL_dcolors = dL_dcolors, .dL_dopacity = dL_dopacity,
                         .dL_dmeans3D = dL_dmeans3D, .dL_dcov3D = dL_dcov3D, .dL_dsh = dL_dsh, .dL_dscales = dL_dscales,
                         .dL_drots = dL_drots};
  bwd_features feat;
  return backward_impl(ctx, stream, prm, BWD_CAMERA, in, radii, geom_buf, binning_buf, img_buf, R, pix, out, feature_side(features, feat),
                       dL_ddistortion, camera);
}

extern "C" int ggd_mark_visible(ggd_ctx* ctx, void* stream, int32_t P, const float* means3D,
                                const float* viewmatrix, const float* projmatrix, uint8_t* present) {
  (void)projmatrix;  // the frustum test only needs view-space z (upstream computes p_proj and ignores it)
  if (!ctx) return GGD_E_INVALID;
  if (P < 0) return ggd_fail(ctx, GGD_E_INVALID, "P < 0");
  if (P == 0) return GGD_OK;
  if (!means3D || !viewmatrix || !present) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mark_visible: NULL pointer");
  return ggd_launch_mark_visible(ctx, static_cast<hipStream_t>(stream), P, means3D, viewmatrix, present);
}

extern "C" int ggd_selftest_lanes(ggd_ctx* ctx, void* stream, const uint64_t* in, uint32_t* out, int32_t n_waves) {
  if (!ctx) return GGD_E_INVALID;
  if (n_waves < 0) return ggd_fail(ctx, GGD_E_INVALID, "n_waves < 0");
  if (n_waves == 0) return GGD_OK;
  if (!in || !out) return ggd_fail(ctx, GGD_E_INVALID, "ggd_selftest_lanes: NULL pointer");
  return ggd_launch_selftest_lanes(ctx, static_cast<hipStream_t>(stream), in, out, n_waves);
}

extern "C" int ggd_debug_unsorted(ggd_ctx* ctx, void* stream, uint64_t* keys, uint32_t* values, int64_t R) {
  if (!ctx) return GGD_E_INVALID;
  if (R < 0 || (size_t)R > ctx->dbg_cap) return ggd_fail(ctx, GGD_E_INVALID, "no debug copy of that size (debug=1?)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (keys && R) GGD_HIP(hipMemcpyAsync(keys, ctx->dbg_keys, (size_t)R * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  if (values && R) GGD_HIP(hipMemcpyAsync(values, ctx->dbg_vals, (size_t)R * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  return GGD_OK;
}
