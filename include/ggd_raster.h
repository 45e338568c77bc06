/*
 * ggd_raster.h -- C ABI of the MI355X-native (gfx950) differentiable 3D-Gaussian-splatting rasterizer.
 *
 * This is the drop-in boundary for the one hot path of fraunhoferhhi/gaussian_gan_decoder: the native
 * module `diff_gaussian_rasterization._C` that the reference imports at
 *   gaussian_splatting/gaussian_renderer/__init__.py:14
 * and drives through `GaussianRasterizer(...)` at
 *   gaussian_splatting/gaussian_renderer/__init__.py:53,87-95 (render) and :139,167-175 (render_simple).
 * The CUDA sources behind that module are an EMPTY, unpinned git submodule in the reference tree
 * (.gitmodules:4-6); the three pybind entry points it would export are replaced here one-to-one:
 *
 *   _C.rasterize_gaussians            ->  ggd_forward_geometry() + ggd_forward_render()
 *   _C.rasterize_gaussians_backward   ->  ggd_backward()
 *   _C.mark_visible                   ->  ggd_mark_visible()
 *
 * Plain pointers and sizes only; no torch types.  All `const float*` / `void*` tensor arguments are DEVICE
 * pointers (HIP, gfx950) unless a comment says "host".  `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  Every function returns 0 on success or a negative GGD_E_* code; the message is available
 * through ggd_last_error().  Nothing here throws.
 *
 * Buffer ownership mirrors the upstream design (geomBuffer / binningBuffer / imgBuffer byte tensors that the
 * autograd function keeps alive between forward and backward): the CALLER allocates them with the sizes
 * returned by ggd_geom_bytes / ggd_binning_bytes / ggd_img_bytes, the library only fills them.  The ctx owns
 * a grow-only scratch workspace (sort ping-pong space, histograms, block sums, a pinned word for the
 * `num_rendered` read-back) and is not re-entrant: one ctx per (device, stream).
 */
#ifndef GGD_RASTER_H
#define GGD_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGD_TILE 16 /* tile edge in pixels (16x16), fixed by the algorithm's contract */

enum {
  GGD_OK = 0,
  GGD_E_INVALID = -1,   /* bad argument (null pointer, negative size, exactly-one-of rule violated, degree) */
  GGD_E_HIP = -2,       /* a HIP runtime call failed */
  GGD_E_NOMEM = -3,     /* workspace allocation failed */
  GGD_E_PREFILTER = -4, /* prefiltered=1 but a Gaussian failed the frustum test (upstream traps here) */
  GGD_E_NODEVICE = -5,  /* no gfx950 device visible */
  GGD_E_CAPACITY = -6   /* ggd_forward: binning_buf capacity below num_rendered (num_rendered is valid: retry) */
};

typedef struct ggd_ctx ggd_ctx;

/* Per-call parameters == the fields of the reference's GaussianRasterizationSettings
 * (constructed at gaussian_renderer/__init__.py:38-51 and :124-137) plus tensor extents. */
typedef struct ggd_params {
  int32_t P;             /* number of Gaussians */
  int32_t M;             /* SH coefficients per channel present in `shs` (stride); 0 when colors_precomp is used */
  int32_t sh_degree;     /* active SH degree D, 0..3 ((D+1)^2 <= M) */
  int32_t width, height; /* image size in pixels */
  float tanfovx, tanfovy;
  float scale_modifier;
  int32_t prefiltered;
  int32_t debug;            /* 1: keep a copy of the unsorted key/value list for ggd_debug_unsorted() */
  const float* viewmatrix;  /* device, 16 floats: world_view_transform flattened row-major (= V^T), cameras.py:85 */
  const float* projmatrix;  /* device, 16 floats: full_proj_transform flattened row-major (= (P V)^T), cameras.py:91 */
  const float* campos;      /* device, 3 floats */
  const float* bg;          /* device, 3 floats */
  int32_t raw_attributes;   /* 1: `scales`, `rotations`, `opacities` are the RAW decoder outputs and the activation
                               prologue of gaussian_model.py:100-121 (exp / L2-normalise (eps 1e-12) / sigmoid) is fused
                               into the per-Gaussian kernels, forward and backward; 0: as upstream */
  int32_t antialiasing;     /* 1: opacity-compensated 2D filter (Mip-Splatting): each Gaussian's opacity is scaled by
                               h = sqrt(max(2.5e-5, det(cov2D) / det(cov2D + 0.3 I))) before blending, forward and
                               backward; the conic, radii and every sort / binning output are unchanged.  The backward
                               then reads `opacities` (NULL -> GGD_E_INVALID).  0: as upstream */
} ggd_params;

/* One record per Gaussian, written by the preprocess kernel and gathered by the blend kernels: exactly what a blended
 * (tile, Gaussian) instance needs, with the per-Gaussian constants of the inner loop formed ONCE here instead of once
 * per instance: the three coefficients of  power = fma(fma(hA, dx, nB*dy), dx, (hC*dy)*dy)  (hA = -A/2, nB = -B,
 * hC = -C/2 are exact rescalings of the conic (A, B, C): A = -2 hA etc. bit for bit), the power-domain cull threshold
 * and the half extents of the axis-aligned box outside of which alpha < 1/255 for sure. */
typedef struct ggd_splat {
  float x, y;               /* pixel-space centre ("means2D" upstream) */
  float hA, nB, hC;         /* -conic.A / 2, -conic.B, -conic.C / 2 (conic = inverse 2D covariance) */
  float thr;                /* ln(1 / (255 opacity)) lowered by a safety margin: power < thr  =>  alpha < 1/255 */
  float opacity;
  float r, g, b;            /* colour after SH evaluation / colors_precomp */
  float ex, ey;             /* half extents of the box {power >= thr}, inflated for fp32 rounding (+inf: keep always) */
} ggd_splat;                /* 48 bytes */

/* Byte offsets of the named arrays inside the caller-owned buffers (for tests / debug taps / bindings). */
typedef struct ggd_geom_view {
  size_t splat;         /* ggd_splat[P] */
  size_t tiles_touched; /* uint32[P] */
  size_t point_offsets; /* uint32[P], inclusive prefix sum of tiles_touched */
  size_t clamped;       /* uint8[P], bit c set <=> colour channel c was clamped at 0 */
  size_t depth_keys;    /* uint32[P]: raw fp32 bits of the view-space depth, 0xFFFFFFFF for culled Gaussians */
  size_t rect;          /* uint32[2*P]: tile rect {minx | maxx << 16, miny | maxy << 16}, zero for culled Gaussians */
  size_t header;        /* uint32[64]: reserved (zeroed) */
  size_t total;
} ggd_geom_view;

typedef struct ggd_binning_view {
  size_t keys;     /* uint64[R] sorted keys:  (tile_id << 32) | depth_bits */
  size_t list;     /* uint32[R] sorted Gaussian indices ("point_list"); ALWAYS at offset 0 of binning_buf, so readers of
                      the list (the backward) do not need to know which R the buffer was laid out for */
  size_t keys_alt; /* uint64[R] ping-pong partner (contents unspecified after the call) */
  size_t list_alt; /* uint32[R] */
  size_t total;
} ggd_binning_view;

typedef struct ggd_img_view {
  size_t ranges;    /* uint32[2*T]: [first, last) into `list` per tile, (0,0) for empty tiles */
  size_t final_T;   /* float[H*W] */
  size_t n_contrib; /* uint32[H*W] */
  size_t total;
} ggd_img_view;

size_t ggd_geom_bytes(int32_t P);
size_t ggd_binning_bytes(int64_t R);
size_t ggd_img_bytes(int32_t width, int32_t height);
int ggd_geom_layout(int32_t P, ggd_geom_view* out);
int ggd_binning_layout(int64_t R, ggd_binning_view* out);
int ggd_img_layout(int32_t width, int32_t height, ggd_img_view* out);

/* Number of key bits the radix sort covers: 32 + msb(#tiles) (11 for 1024 tiles, 13 for 4096). */
int ggd_sort_bits(int32_t width, int32_t height);

ggd_ctx* ggd_create(int device);
void ggd_destroy(ggd_ctx* ctx);
const char* ggd_last_error(ggd_ctx* ctx); /* ctx may be NULL: returns the last creation error */
const char* ggd_version(void);

/*
 * Forward, phase 1 (per Gaussian): frustum cull, cov3D, EWA cov2D, conic, radius, tile rect, SH->RGB;
 * inclusive scan of tiles_touched; reads the total back ("num_rendered", one host sync on `stream`).
 * Exactly one of {shs, colors_precomp} and exactly one of {scales+rotations, cov3D_precomp} must be non-NULL.
 *   means3D[P,3] opacities[P] shs[P,M,3] colors_precomp[P,3] scales[P,3] rotations[P,4](w,x,y,z) cov3D_precomp[P,6]
 *   geom_buf : ggd_geom_bytes(P) bytes, written     radii : int32[P], written     num_rendered : HOST out
 */
int ggd_forward_geometry(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                         const float* means3D, const float* shs, const float* colors_precomp,
                         const float* opacities, const float* scales, const float* rotations,
                         const float* cov3D_precomp,
                         void* geom_buf, int32_t* radii, int64_t* num_rendered);

/*
 * Forward, phase 2 (per instance / per tile): duplicateWithKeys, stable radix sort of (tile|depth) keys,
 * identifyTileRanges, front-to-back alpha blend.  No host sync.
 *   binning_buf : ggd_binning_bytes(num_rendered)   img_buf : ggd_img_bytes(W,H)   out_color : float[3,H,W]
 */
int ggd_forward_render(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                       const void* geom_buf, int64_t num_rendered,
                       void* binning_buf, void* img_buf, float* out_color);

/*
 * Forward in ONE call with a caller-chosen binning capacity (instances): geometry + render are enqueued back to back,
 * so the GPU does not idle while num_rendered travels to the host (the two-phase form above stalls the stream for that
 * round trip).  On the speculative route the call returns as soon as num_rendered has ARRIVED -- the binning and blend
 * kernels may still be running: out_color and the buffers are ordered on `stream` like the result of any asynchronous
 * launch (upstream's forward likewise returns with its render kernels in flight); synchronise the stream before reading
 * them from the host or from another stream.  binning_buf must hold ggd_binning_bytes(capacity).  Returns
 * GGD_E_CAPACITY (with *num_rendered set) when capacity < num_rendered: call again with a larger buffer.  ggd_backward
 * takes the returned num_rendered (the sorted list is at offset 0 of binning_buf for every capacity).  ggd_forward_can_speculate
 * tells whether the call will take the speculative route (tile-binning path) for that capacity.
 */
int ggd_forward(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                const float* scales, const float* rotations, const float* cov3D_precomp,
                void* geom_buf, int32_t* radii, void* binning_buf, int64_t capacity, void* img_buf,
                float* out_color, int64_t* num_rendered);

/*
 * The same forward in two halves, for hosts that keep several frames in flight (one context + stream per frame slot: the
 * latency-bound front of frame k + 1 -- per-Gaussian kernel, depth sort, binning -- runs under the blend of frame k).
 * ggd_forward_enqueue launches the whole frame and returns at once; it needs the speculative route (ggd_forward_can_speculate,
 * P > 0, capacity > 0).  ggd_forward_collect, called any time later on the same context (typically when the slot comes round
 * again, the frame long finished), returns that frame's num_rendered -- or GGD_E_CAPACITY with it, in which case the outputs
 * are not valid and the frame has to be rendered again with a larger buffer.  At most one frame per context may be pending:
 * while one is, ggd_forward / ggd_forward_geometry / ggd_forward_render / ggd_forward_enqueue on that context return
 * GGD_E_INVALID (the pending frame's verification state lives on the context).  The buffers, the camera matrices and the other
 * pointers of `prm` must stay valid until it is collected.
 */
int ggd_forward_enqueue(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                        const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                        const float* scales, const float* rotations, const float* cov3D_precomp,
                        void* geom_buf, int32_t* radii, void* binning_buf, int64_t capacity, void* img_buf, float* out_color);
int ggd_forward_collect(ggd_ctx* ctx, void* stream, int64_t* num_rendered);
int ggd_forward_can_speculate(ggd_ctx* ctx, const ggd_params* prm, int64_t capacity);

/*
 * Backward.  Consumes the three buffers of the matching forward plus the original inputs and dL/d(out_color).
 * All nine gradient outputs are fully written (zero-filled then accumulated) by the library:
 *   dL_dmeans2D[P,3] (xy = NDC-scaled screen gradient, z = 0)   dL_dcolors[P,3]   dL_dopacity[P]
 *   dL_dmeans3D[P,3]   dL_dcov3D[P,6]   dL_dsh[P,M,3] (may be NULL iff M == 0)   dL_dscales[P,3]   dL_drots[P,4]
 * dL_dconic is internal scratch.
 */
int ggd_backward(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                 const float* means3D, const float* shs, const float* colors_precomp,
                 const float* opacities /* only read when prm->raw_attributes or prm->antialiasing */,
                 const float* scales, const float* rotations, const float* cov3D_precomp,
                 const int32_t* radii,
                 const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                 const float* dL_dpix,
                 float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                 float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots);

/*
 * Depth and alpha planes (opt-in extension; the entry points above are unchanged by it).  Per pixel p, over the same
 * contributors, skip rules and stop rule as the colour:
 *   depth[p] = sum_i alpha_i T_i z_i   (z_i = Gaussian i's view-space depth, the value the depth sort orders by; background 0;
 *                                       the expected depth is depth / alpha)
 *   alpha[p] = 1 - final_T[p]          (the pixel's opacity)
 * out_depth, out_alpha : float[H,W] each, written (both required).  out_color, radii, the three buffers and num_rendered are
 * bit-identical to those of the plain call.
 *   ggd_forward_aux        == ggd_forward (speculative route, its re-render and GGD_E_CAPACITY included) + the two planes
 *   ggd_forward_render_aux == ggd_forward_render + the two planes (phase 1 is ggd_forward_geometry, unchanged)
 *   ggd_backward_aux       == ggd_backward + dL_ddepth[H,W], dL_dalpha[H,W] (device; NULL = zero).  The depth term reaches
 *                             dL_dmeans3D through z (dz/dmean = row 2 of the view matrix), the alpha term every input through
 *                             the final transmittance.  Runs the quarter form of the backward blend whatever
 *                             GGD_OPT_BLEND_SPLIT says (the depth / alpha backward has no tile form).
 */
int ggd_forward_aux(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                    const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                    const float* scales, const float* rotations, const float* cov3D_precomp,
                    void* geom_buf, int32_t* radii, void* binning_buf, int64_t capacity, void* img_buf,
                    float* out_color, float* out_depth, float* out_alpha, int64_t* num_rendered);
int ggd_forward_render_aux(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                           const void* geom_buf, int64_t num_rendered,
                           void* binning_buf, void* img_buf, float* out_color, float* out_depth, float* out_alpha);
int ggd_backward_aux(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                     const float* means3D, const float* shs, const float* colors_precomp,
                     const float* opacities /* only read when prm->raw_attributes or prm->antialiasing */,
                     const float* scales, const float* rotations, const float* cov3D_precomp,
                     const int32_t* radii,
                     const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                     const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                     float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                     float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots);

/*
 * Absolute screen-space gradients (opt-in extension, the densification signal of AbsGS; ggd_backward and ggd_backward_aux
 * are unchanged by it).  ggd_backward_abs == ggd_backward_aux + one more output:
 *   dL_dmeans2D_abs : float[P,3], written in full = (0.5 W sum_q |g_x(q,i)|, 0.5 H sum_q |g_y(q,i)|, 0), where g_x, g_y are
 *                     the per-pixel terms whose SIGNED sums are dL_dmeans2D[i] -- same contributors, same skip and stop rules,
 *                     the depth / alpha terms included when dL_ddepth / dL_dalpha are given; zeros for culled Gaussians.
 * dL_ddepth and dL_dalpha may both be NULL: the other eight gradients are then those of ggd_backward (the plain arithmetic),
 * with either they are those of ggd_backward_aux.  Same validation as ggd_backward_aux (GGD_E_INVALID for a NULL
 * dL_dmeans2D_abs).  Runs the quarter form of the backward blend whatever GGD_OPT_BLEND_SPLIT says.  Like every blend
 * gradient the sums are float atomics: not bit-reproducible from run to run.
 */
int ggd_backward_abs(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                     const float* means3D, const float* shs, const float* colors_precomp,
                     const float* opacities /* only read when prm->raw_attributes or prm->antialiasing */,
                     const float* scales, const float* rotations, const float* cov3D_precomp,
                     const int32_t* radii,
                     const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                     const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                     float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                     float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots,
                     float* dL_dmeans2D_abs);

/*
 * Feature maps (opt-in extension; every entry point above is unchanged by it).  C per-Gaussian channels, 1 <= C <=
 * GGD_FEATURES_MAX_CHANNELS, blended over exactly the contributors of a finished colour render -- front to back, same skip
 * rules, same stop -- with the colour pass's own alpha_i and T_i (so prm->antialiasing's compensated opacity and
 * prm->raw_attributes' activations are in them: the pass reads the geometry buffer's per-Gaussian records and is indifferent to
 * how they were produced):
 *   F[c][p] = sum_i alpha_i T_i f[i][c] + final_T[p] * feature_bg[c]          c = 0 .. C - 1
 * features     : float[P,C] (device).  feature_bg : float[C] (device) or NULL = zeros; it gets no gradient.
 * out_features : float[C,H,W], written in full.
 *   ggd_forward_features   one launch behind a completed forward (ggd_forward / ggd_forward_render or their _aux forms, same
 *                          ctx, stream-ordered), on that forward's three buffers and its num_rendered; prm as in that forward.
 *                          The walk of a pixel is bounded by the forward's stored contributor count; alpha is recomputed with
 *                          the colour kernels' own expressions for the GGD_OPT_EXP_MODE / GGD_OPT_BLEND_CULL in effect (which
 *                          must be the forward's), so every (pixel, Gaussian) pair is in or out as it was in the colour.
 *   ggd_backward_features  == ggd_backward_aux's arguments + features, C, feature_bg, dL_dfeatmap[C,H,W] (device) before the eight
 *                          gradient arrays and dL_dfeatures[P,C] behind them.  One more launch between the blend backward and
 *                          the per-Gaussian backward: the feature map's dL/dconic, dL/dopacity and dL/dmean2D are ADDED to
 *                          those of the colour (and depth / alpha) maps in the library's accumulator records, so the eight
 *                          arrays hold the gradients of all maps together; dL_dfeatures is written in full (zeros for
 *                          culled Gaussians).  The depth / alpha terms run exactly when dL_ddepth or dL_dalpha is given;
 *                          without both the colour part is ggd_backward's arithmetic.
 * GGD_E_INVALID with a message: C outside 1 .. GGD_FEATURES_MAX_CHANNELS; a NULL features (with P > 0), out_features,
 * dL_dfeatmap or dL_dfeatures.  P = 0 and num_rendered = 0 are valid: num_rendered = 0 gives F = feature_bg everywhere and
 * all-zero feature gradients.  Like every blend gradient the sums are float atomics: not bit-reproducible from run to run.
 * GGD_FEATURES_ROUND: list entries both kernels consume per round (tests place lists at its boundaries).
 */
#define GGD_FEATURES_MAX_CHANNELS 32
#define GGD_FEATURES_ROUND 64
int ggd_forward_features(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                         const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                         const float* features, int32_t C, const float* feature_bg /* NULL = 0 */, float* out_features);
int ggd_backward_features(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                          const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities /* only read when prm->raw_attributes or prm->antialiasing */,
                          const float* scales, const float* rotations, const float* cov3D_precomp,
                          const int32_t* radii,
                          const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                          const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                          const float* features, int32_t C, const float* feature_bg, const float* dL_dfeatmap,
                          float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                          float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots,
                          float* dL_dfeatures);

/*
 * Depth-distortion map (opt-in extension, the distortion loss of Mip-NeRF 360 / 2DGS; every entry point above is unchanged by
 * it).  Per pixel, over exactly the contributors of a finished colour render, in list order k = 1 .. n, with w_k = alpha_k T_k
 * and z_k the view-space depth of the depth plane (raw, not normalised):
 *   D[p] = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_k w_k (z_k A_{k-1} - B_{k-1}),   A_k = sum_{j<=k} w_j,  B_k = sum_{j<=k} w_j z_j
 * The background does not enter; a pixel with fewer than two contributors has D = 0.
 * out_distortion : float[H,W], written in full.
 *   ggd_forward_distortion   one launch behind a completed forward (same ctx, stream-ordered), on that forward's three buffers
 *                            and its num_rendered; prm, GGD_OPT_EXP_MODE and GGD_OPT_BLEND_CULL as in that forward (as for
 *                            ggd_forward_features).
 *   ggd_backward_distortion  == ggd_backward_aux's arguments + dL_ddistortion[H,W] (device) + `features`.  One more launch
 *                            between the blend backward and the per-Gaussian backward ADDS the map's dL/dconic, dL/dopacity,
 *                            dL/dmean2D and dL/dz to the library's accumulator records; dL/dz reaches dL_dmeans3D as the depth
 *                            plane's does, so the depth / alpha instances always run (dL_ddepth and dL_dalpha may be NULL).
 *                            At equal depths the gradient in z is the list order's (the limit of the later record lying behind).
 *                            features: NULL, or the feature map's side of ggd_backward_features as one bundle -- the call then
 *                            does that entry point's work as well (ggd_backward_features keeps its signature).
 * GGD_E_INVALID with a message: a NULL out_distortion, img_buf or dL_ddistortion; NULL geom_buf / binning_buf with
 * num_rendered > 0; ggd_backward_features' refusals for the bundle.  num_rendered = 0 gives D = 0 everywhere.
 */
typedef struct ggd_feature_side {
  const float* features;      /* [P,C] */
  int32_t C;
  const float* feature_bg;    /* [C] or NULL = zeros */
  const float* dL_dfeatmap;   /* [C,H,W] */
  float* dL_dfeatures;        /* [P,C], written in full */
} ggd_feature_side;
int ggd_forward_distortion(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                           const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                           float* out_distortion);
int ggd_backward_distortion(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                            const float* means3D, const float* shs, const float* colors_precomp,
                            const float* opacities /* only read when prm->raw_attributes or prm->antialiasing */,
                            const float* scales, const float* rotations, const float* cov3D_precomp,
                            const int32_t* radii,
                            const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                            const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                            float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                            float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots,
                            const float* dL_ddistortion, const ggd_feature_side* features /* NULL = no feature map */);

/*
 * Contribution statistics (opt-in extension; every entry point above is unchanged by it): which Gaussians a frame used, and how
 * much -- what pruning and compaction of a trained model rank by (hit counts, summed blend weights, the largest blend weight).
 * Over exactly the (pixel, Gaussian) pairs the finished colour render blended, with w = alpha T the colour pass's own weight of
 * the pair (bit for bit, as for ggd_forward_features), per Gaussian i:
 *   stats[i][0] += rint(w * 2^GGD_CONTRIB_SCALE_LOG2)   the summed weight in fixed point (ties to even: each term is within
 *                                                       2^-25 of w; the scaling is exact in fp32)
 *   stats[i][1] += 1                                    the number of pixels that blended i
 *   stats[i][2]  = max(stats[i][2], bits of w)          the largest weight: w > 0, so the fp32 bit pattern, zero-extended, orders
 *                                                       as the value does
 * stats : int64[P,3] (device, 8-byte aligned), ACCUMULATED in place: zero it once, then call per frame and per camera.  Rows of
 * Gaussians no pixel blended are neither read nor written.  All three updates are integer atomics: the result does not depend on
 * the order of arrival and is bit-identical from run to run.
 *   ggd_contribution   one launch behind a completed forward (ggd_forward / ggd_forward_render or their _aux forms, same ctx,
 *                      stream-ordered), on that forward's three buffers and its num_rendered; prm, GGD_OPT_EXP_MODE and
 *                      GGD_OPT_BLEND_CULL as in that forward (as for ggd_forward_features).  Forward only: it has no gradient and
 *                      changes nothing a backward reads.
 * GGD_E_INVALID with a message, before any launch: a NULL stats with P > 0; a stats that is not 8-byte aligned; a NULL img_buf;
 * NULL geom_buf / binning_buf with num_rendered > 0.  P = 0 and num_rendered = 0 are valid and change nothing.
 */
#define GGD_CONTRIB_SCALE_LOG2 24
int ggd_contribution(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                     const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                     int64_t* stats /* [P][3], ACCUMULATED in place */);

/*
 * Camera gradients (opt-in extension; every entry point above is unchanged by it): the backward also differentiates the frame in
 * prm->viewmatrix, prm->projmatrix and prm->campos.
 *   ggd_backward_camera  == ggd_backward_distortion's arguments + `camera`.  dL_ddistortion and `features` may be NULL, and so may
 *                        dL_ddepth / dL_dalpha: the call does the work of ggd_backward (all four NULL), ggd_backward_aux (a depth
 *                        or alpha gradient), ggd_backward_features (the bundle) or ggd_backward_distortion (the map's gradient, with
 *                        or without the bundle) as given, and then two more launches on the same accumulator records.
 * Entry k of each gradient is the derivative with respect to flat entry k of the input, m[4c + r] = row r, column c of the maths
 * matrix.  Per Gaussian with radii > 0, p = (p0, p1, p2, 1), in the per-Gaussian backward's quantities:
 *   dL_dviewmatrix[4c + r] += dt_r p_c (r = 0..2; dt the gradient of t = V p through the EWA Jacobian, with the depth plane's and
 *                             the distortion map's dL/dz on dt_2) and, through W in T = J W, for c = 0..2:
 *                             [4c + 0] += J00 dT[0][c], [4c + 1] += J11 dT[1][c], [4c + 2] += J02 dT[0][c] + J12 dT[1][c]
 *   dL_dprojmatrix[4c + r] += dh_r p_c for r = 0, 1, 3; dh = (m_w g0, m_w g1, -, -(mul1 g0 + mul2 g1)), g = dL_dmeans2D
 *   dL_dcampos             -= the term the SH view direction adds to dL_dmeans3D (zero at degree 0 and with colors_precomp)
 * The bottom row of the view matrix and row 2 of the projection matrix are read by no kernel: exactly 0.  The conventions of the
 * published backward hold (1 / (det^2 + 1e-7), the half dB slot, clamped x, y independent of z): it is the derivative of the same
 * surrogate dL_dmeans3D is.  Culling, radii and tile decisions carry no gradient, and tanfovx / tanfovy get none.
 * All three arrays are device pointers and are written in full, zeros included; P == 0 or num_rendered == 0 writes zeros.  The
 * sums are reduced in a fixed order without float atomics: given the same accumulator records (which the blend's float atomics
 * fill) they are bit-identical from run to run.
 * GGD_E_INVALID with a message: a NULL `camera` or a NULL member; the refusals of the entry point whose work the call does.
 */
typedef struct ggd_camera_grads {
  float* dL_dviewmatrix;   /* [16] */
  float* dL_dprojmatrix;   /* [16] */
  float* dL_dcampos;       /* [3] */
} ggd_camera_grads;
int ggd_backward_camera(ggd_ctx* ctx, void* stream, const ggd_params* prm,
                        const float* means3D, const float* shs, const float* colors_precomp,
                        const float* opacities /* only read when prm->raw_attributes or prm->antialiasing */,
                        const float* scales, const float* rotations, const float* cov3D_precomp,
                        const int32_t* radii,
                        const void* geom_buf, const void* binning_buf, const void* img_buf, int64_t num_rendered,
                        const float* dL_dpix, const float* dL_ddepth, const float* dL_dalpha,
                        float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity,
                        float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots,
                        const float* dL_ddistortion /* NULL = no distortion map */,
                        const ggd_feature_side* features /* NULL = no feature map */,
                        const ggd_camera_grads* camera);

/* present[i] = 1 iff Gaussian i passes the view-space z > 0.2 frustum test. */
int ggd_mark_visible(ggd_ctx* ctx, void* stream, int32_t P, const float* means3D,
                     const float* viewmatrix, const float* projmatrix, uint8_t* present);

/* Debug tap (prm->debug = 1 on the preceding ggd_forward_render): copies the UNSORTED duplicateWithKeys output
 * to device buffers keys[R] / values[R] supplied by the caller.  Either pointer may be NULL. */
int ggd_debug_unsorted(ggd_ctx* ctx, void* stream, uint64_t* keys, uint32_t* values, int64_t num_rendered);

/* Self-test of the front-end kernels' cross-lane primitives (register forms: DPP, lane-block swaps, v_readlane) against the
 * shuffle forms they replaced.  One wave per 64 input words: lane l of wave w takes in[64 w + l] (x = its low 32 bits; the whole
 * word is row l of a 64 x 64 bit matrix) and writes GGD_LANES_SELFTEST_WORDS words at out[(64 w + l) * GGD_LANES_SELFTEST_WORDS]:
 *   0, 1      inclusive scan of x over the lanes (uint32): new, shuffle form          2, 3   the same as int
 *   4, 5      sum of x over the wave (every lane)                                     6, 7   maximum of x (unsigned)
 *   8 .. 13   x of lane l ^ 1, 2, 4, 8, 16, 32: new                                   14 .. 19   shuffle form
 *   20 .. 83  x of lane c, c = 0 .. 63: new                                           84 .. 147  shuffle form
 *   148, 149  column l of the bit matrix (low, high word): new                        150, 151   shuffle form
 *   152, 153  x + x of lane l ^ 16, l ^ 32 (new)      154, 155   maximum / sum of x with the result in lane 63 only (there: new)
 * in: n_waves * 64 words, out: n_waves * 64 * GGD_LANES_SELFTEST_WORDS words, both on the device. */
#define GGD_LANES_SELFTEST_WORDS 156
int ggd_selftest_lanes(ggd_ctx* ctx, void* stream, const uint64_t* in, uint32_t* out, int32_t n_waves);

/* Tuning / experiment knobs (do not change results beyond the documented tolerances).  Returns GGD_E_INVALID for an
 * unknown option or value. */
enum {
  GGD_OPT_EXP_MODE = 0,   /* blend exp(): 0 = ocml expf (<=1 ulp), 1 = native 2^(x*log2e) (fast, ~3 ulp),
                             2 = compensated 2^x (v_exp_f32 + product-residual correction, 1-2 ulp), in both blend kernels;
                             3 (default) = 1 in the forward, 2 in the backward: at 1 M Gaussians / 1024^2 the image stays within
                             5.4e-7 of the fp32 oracle (2: 3.6e-7; the bar is 1e-5) and the forward blend is 7 % faster; the
                             backward's error budget needs the 1-2 ulp class (mode 1 there: gradients 3-4 x outside it) */
  GGD_OPT_BLEND_CULL = 1, /* 1 (default) = skip records whose alpha cannot reach 1/255 anywhere in the tile */
  GGD_OPT_BINNING = 2,    /* how the per-tile sorted lists are built (results are identical):
                             0 = duplicateWithKeys + 64-bit (tile|depth) radix sort + identifyTileRanges,
                             3 = depth-sort the Gaussians once, then TWO 1-D stable binning passes (tile rows, then
                                 columns; grids up to 255 x 255 tiles = 4080 x 4080 pixels, falls back to 0 beyond),
                             2 = alias of 3 (the single-level tile binning it used to select was removed: slower than 3
                                 on every grid 3 supports),
                             1 (default) = auto: 3 wherever it applies, else 0.
                             debug=1 (key taps) always uses 0 */
  GGD_OPT_BLEND_SPLIT = 3, /* backward blend (the forward always runs four 8x8 quarter waves per tile, one pixel per
                             lane): 3 = the four quarter waves of a tile in one workgroup, per-record sums combined in LDS;
                             4 = four independent quarter waves per tile; 1 (default) = auto (= 4 since round 6: equal or faster on every grid measured);
                             0, 2 = aliases of 3 (the one-wave and two-wave forms they selected were removed).  Backward sums
                             differ only in their fp32 summation order. */
  GGD_OPT_FOLD = 4,       /* single-call forward on the tile-binning path: 1 (default) = the per-Gaussian kernel also builds the
                             depth sort's digit histograms and the first step of the offsets scan (no histogram launch);
                             0 = separate histogram launch.  Results are identical. */
  GGD_OPT_MSD_SORT = 5,   /* 1 (default): once the kept depth keys' ranges of 8 single-call frames are known, the depth sort of the
                             single-call forward runs as TWO launches over a speculated key window fitted to those ranges (one
                             partition by (key - window start) >> shift without any dependency between tiles + an in-LDS finish
                             per bucket) instead of three or four onesweep passes; verified by every frame's own front end (no
                             kept key outside the window, no bucket above the finish kernel's capacity), a frame it does not hold
                             for is re-rendered by the ordinary path and its range joins the window.  0 = never.  Results are
                             identical.  Setting this option or GGD_OPT_FOLD (to any value) restarts the speculation state. */
  GGD_OPT_PREPROCESS_WGS = 6, /* workgroups of the per-Gaussian forward kernel, each of which strides over the 256-Gaussian tiles:
                             0 (default) = automatic (a fixed number per compute unit), n > 0 = exactly min(n, tiles).  Results are
                             identical; for timing experiments, and so that a small input can put many tiles on one workgroup. */
  GGD_OPT_L1_COUNTED = 7, /* frames of the two-launch depth sort on grids of up to 64 x 64 tiles: 1 (default) = the sort's finish
                             launch also counts every bucket's row entries, and level 1 of the row binning sums those finished rows
                             instead of looking back over the chunks of its own launch; 0 = the look-back kernel.  Results are
                             identical; for A/B timing and tests. */
  GGD_OPT_COUNT
};
#define GGD_PREPROCESS_WGS_MAX (1 << 20)
int ggd_set_option(ggd_ctx* ctx, int option, int value);
/* Debug: blend work counters of the NEXT forward calls: out[0]=records visited, [1]=records culled by the wave-level
 * test, [2]=lanes with a candidate pixel (summed over visited records), [3]=candidate pixels, [4]=sum of list lengths,
 * [5]=the part of [1] that was staged and then rejected by the whole wave inside the blend loop.
 * enable=1 starts (and zeroes) counting, enable=0 stops; out (host, 6 x uint64) may be NULL.
 * enable=2 records, instead of the counters, a per-wave timeline of the next forward blend: ggd_blend_timeline copies, for
 * the first `waves` workgroups of that launch, 3 x uint64 each: start and end on the device's 100 MHz constant clock, and
 * (list length << 32 | list entries gathered before the wave's pixels were all finished).  (The counters are same-address
 * atomics and stretch the kernel; the timeline is one plain store per wave.) */
int ggd_blend_stats(ggd_ctx* ctx, int enable, unsigned long long* out);
/* ... and of the backward blends (quarter form) that ran since ggd_blend_stats(ctx, 1, ..) started counting; call BEFORE stopping:
 * out[0]=list entries walked (sum over quarter waves of the positions up to the wave's last contributor), [1]=records staged after
 * the pre-cull, [2]=staged records some pixel of the wave still needed, [3]=records at least one pixel blended (one 9-sum wave
 * reduction each), [4]=live lanes of those, [5]=rows flushed = 36-byte atomic spans, [6]=gather rounds, [7]=waves with work. */
int ggd_blend_backward_stats(ggd_ctx* ctx, unsigned long long* out);
int ggd_blend_timeline(ggd_ctx* ctx, unsigned long long* out, int waves);
int ggd_get_option(ggd_ctx* ctx, int option);
/* Read-only counters through ggd_get_option (single-call forward with GGD_OPT_FOLD = 1): the depth keys' top byte is constant in
 * most scenes, which makes the fourth sort pass an empty launch; after 8 such frames in a row it is not launched, every
 * frame's own histogram says whether that held, and a frame for which it did not is binned and blended again before
 * ggd_forward returns (results are identical either way). */
enum {
  GGD_STAT_FLAT_STREAK = 100,   /* consecutive frames whose top depth digit was constant */
  GGD_STAT_SORT_RERUNS = 101,   /* frames re-rendered because the speculated short form of the depth sort did not hold */
  GGD_STAT_MSD_FRAMES = 102,    /* frames whose depth sort ran as two launches (GGD_OPT_MSD_SORT) */
  GGD_STAT_SCAN_IN_SCATTER_FRAMES = 103,  /* frames (binning passes) whose row binning ran without its level-2 scan launch: the per-Gaussian
                                             kernel counted the instances per tile row, the scatter workgroups form their tile starts */
  GGD_STAT_L1_COUNTED_FRAMES = 104        /* frames (binning passes) whose level 1 took its row counts from the sort's finish launch
                                             (GGD_OPT_L1_COUNTED) */
};

/*
 * Tri-plane feature gather of the per-point decoder (input side of the raster path; replaces the three torch ops
 * sample_from_planes -> grid_sample -> mean(0) of main/decoder_models/sequential_decoder_reverse.py:42-57 and
 * base_decoder.py:22):  out[n,:] = mean over the 3 EG3D planes of the bilinear sample (zero padding,
 * align_corners = False) at (2/box_warp) * pos[n].  planes_cl is CHANNEL-LAST [3][H][W][C], C a power of two <= 64.
 * The backward zero-fills dplanes_cl [3][H][W][C] and scatter-adds dout[N,C]; positions receive no gradient.
 */
int ggd_triplane_forward(ggd_ctx* ctx, void* stream, const float* planes_cl, int32_t C, int32_t H, int32_t W,
                         const float* pos, int32_t N, float box_warp, float* out);
int ggd_triplane_backward(ggd_ctx* ctx, void* stream, int32_t C, int32_t H, int32_t W, const float* pos, int32_t N,
                          float box_warp, const float* dout, float* dplanes_cl);

/*
 * The PanoHead form of the same gather: every plane is a C x D "tri-grid" sampled with a 3-D grid_sample (trilinear,
 * zero padding, align_corners = False) at all three projected coordinates (PanoHead/training/volumetric_rendering/
 * renderer.py:47-58, chosen at sequential_decoder_reverse.py:42-50 when the generator has `triplane_depth`).
 * grids_cl is CHANNEL-LAST [3][D][H][W][C]; axes: 0 = EG3D plane axes, 1 = PanoHead plane axes (they differ in the third
 * plane).  out[n,:] = mean over the 3 grids.  The backward zero-fills dgrids_cl and scatter-adds dout[N,C].
 */
int ggd_trigrid_forward(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                        int32_t axes, const float* pos, int32_t N, float box_warp, float* out);
int ggd_trigrid_backward(ggd_ctx* ctx, void* stream, int32_t C, int32_t D, int32_t H, int32_t W, int32_t axes,
                         const float* pos, int32_t N, float box_warp, const float* dout, float* dgrids_cl);

/*
 * The general form of the four entries above (they are thin wrappers of it): D = 0 selects the 2-D tri-plane form
 * (axes must be 0), D >= 1 the tri-grid.  `mod` (NULL = none): a per-(depth, channel) modulation [max(D,1)][C] of the
 * planes -- what is sampled is fl(texel * mod), i.e. the gather of `planes * code[None, :, None, None]` without that
 * product ever being materialised (the training step's stand-in for per-scene planes of a shared backbone,
 * main/decoder_models/sequential_decoder_reverse.py:89-99); the scatter returns the gradient w.r.t. the UNMODULATED
 * planes.  accumulate != 0: dgrids_cl is added to instead of zero-filled first (several scenes into one gradient
 * buffer).  Large N (>= 49152 points, C in {16, 32, 64}): the (point, plane) items are sorted by cell and summed in
 * registers per run of equal cells, one group of atomics per run; otherwise one atomic per (point, tap, channel).
 */
int ggd_planes_gather(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                      int32_t axes, const float* mod, const float* pos, int32_t N, float box_warp, float* out);
int ggd_planes_scatter(ggd_ctx* ctx, void* stream, int32_t C, int32_t D, int32_t H, int32_t W, int32_t axes,
                       const float* mod, const float* pos, int32_t N, float box_warp, const float* dout,
                       float* dgrids_cl, int32_t accumulate);

/*
 * GPU iso-surface point sampler -- the position generator of the decoder training step, replacing the CPU marching
 * cubes + trimesh + D2H/H2D hop of main/decoder_utils/target_dataloader.py:96-118,172-176: density grid sigma[n][n][n]
 * ([x][y][z], z fastest, main/marching_cube/sample.py:15-17) -> iso-surface at `level` (reference: 10) by marching
 * tetrahedra -> num_points positions, point i on face (i mod F) of pass (i div F) with barycentric weights rand(3)/sum
 * (:104-110), in the reference's units (index / n - 0.5, :99-101), scaled by clip(1 + thickness * N(0,1), 0, 1)
 * (:113-116).  No host sync: the face count F stays on the device (*num_faces, a DEVICE uint32; 0 -> positions are
 * zero-filled).  Pure function of (sigma, level, seed).  tmp: ggd_surface_tmp_bytes(n) bytes of device scratch.
 * 2 <= n <= 711: face numbers are uint32 and a cell emits up to 12 faces, 12 (n - 1)^3 < 2^32 up to n = 711; any other n
 * (and num_points < 0, a NULL pointer, a short tmp) is refused before anything is launched, and ggd_surface_tmp_bytes
 * returns 0 for it.
 */
size_t ggd_surface_tmp_bytes(int32_t n);
int ggd_surface_sample(ggd_ctx* ctx, void* stream, const float* sigma, int32_t n, float level, int32_t num_points,
                       float thickness, uint64_t seed, float* positions, uint32_t* num_faces, void* tmp,
                       size_t tmp_bytes);

/*
 * Fused per-point decoder, inference (bf16 MFMA, fp32 accumulate): the 5 chained `Decoder` MLPs of
 * main/decoder_models/sequential_decoder_reverse.py:68-85 in ONE launch (the other two decoder types: THE DECODER CHAINS below).
 *   feat  [N,32]  mean-of-planes features (ggd_triplane_forward)      pos [N,3] positions
 *   packed_weights : ggd_decoder_packed_bytes() bytes, the LDS image of the 5 heads (bf16 weight rows pre-permuted to
 *                    the MFMA operand order + fp32 biases; built by gaussian_gan_decoder_amd.fused_decoder.pack_weights)
 *   attrs [N,16]  out: [0..2] color, [3] opacity, [4..7] rotation, [8..10] scale (= -softplus(s+5)-2.5; - 2 in chains 1, 2),
 *                      [11..13] xyz (= head*0.01 + pos), [14..15] zero
 */
size_t ggd_decoder_packed_bytes(void);
/* Build the weight images on the device in ONE launch: params40 = HOST array of 40 DEVICE pointers, per head (colour,
 * opacity, rotation, scale, xyz) W1 b1 W2 b2 W3 b3 W4 b4 as torch.nn.Linear stores them (fp32, [out][in] row-major;
 * in = 35, 38, 39, 43, 46, out = 3, 1, 4, 3, 3); packed: ggd_decoder_packed_bytes(), packed_t (may be NULL):
 * ggd_decoder_packed_t_bytes().  Training calls it after every optimizer step. */
int ggd_decoder_pack(ggd_ctx* ctx, void* stream, const float* const* params40, void* packed, void* packed_t);
/* attrs rows [N][16] -> the five contiguous arrays the rasterizer entry takes (what the reference assigns to the GaussianModel,
 * main/train_pano2gaussian_decoder.py:223-227), and the gradients back into rows (a NULL array = zeros): one pass each way. */
int ggd_attrs_split(ggd_ctx* ctx, void* stream, const float* attrs, int64_t N, float* xyz, float* scale, float* rotation,
                    float* opacity, float* color);
int ggd_attrs_merge(ggd_ctx* ctx, void* stream, int64_t N, const float* dxyz, const float* dscale, const float* drotation,
                    const float* dopacity, const float* dcolor, float* dattrs);
int ggd_decoder_forward(ggd_ctx* ctx, void* stream, const float* feat, const float* pos, int32_t N,
                        const void* packed_weights, float* attrs);

/*
 * THE DECODER CHAINS.  The reference selects one of three decoders (main/train_pano2gaussian_decoder.py:45,170-192); the
 * same kernels run all three, as compile-time instances.  A chain is the ORDER in which the five attributes are decoded and
 * what each head sees behind the 32 plane features and the position (its "info" slots 3 .. 3 + n_extra: the outputs of the
 * heads executed before it, in execution order -- the reference's own torch.concat order, so W1 is taken as it is):
 *   chain                            execution order                          n_extra          first-layer widths   scale
 *   GGD_CHAIN_SEQUENTIAL_REVERSED    colour, opacity, rotation, scale, xyz    0, 3, 4, 8, 11   35, 38, 39, 43, 46   -softplus(s+5) - 2.5
 *   GGD_CHAIN_SEQUENTIAL             xyz, scale, rotation, opacity, colour    0, 3, 6, 10, 11  35, 38, 41, 45, 46   -softplus(s+5) - 2
 *   GGD_CHAIN_PARALLEL               xyz, scale, rotation, opacity, colour    0, 0, 0, 0, 0    35 x 5               -softplus(s+5) - 2
 * (main/decoder_models/sequential_decoder_reverse.py, sequential_decoder.py:27-84, parallel_decoder.py:27-80).
 * The attrs[N,16] row is THE SAME for every chain (colour 0..2, opacity 3, rotation 4..7, activated scale 8..10, xyz 11..13,
 * 14..15 zero): an attribute keeps its columns and its activation wherever it executes.  In GGD_CHAIN_SEQUENTIAL info slots
 * 3..5 read columns 11..13, 6..8 read 8..10, 9..12 read 4..7 and 13 reads column 3.
 * EVERYTHING PER HEAD IS INDEXED BY EXECUTION POSITION: params40 is passed in the chain's execution order (for chains 1 and 2:
 * xyz, scale, rotation, opacity, colour), and so are the head slots of the weight images, of zbuf / dzbuf, of dout[h] and of
 * the weight-gradient blocks; dinfo[N,16] is in the chain's slot order (slots 0..2 position, 3 + k the k-th chained input).
 * Backward: a head adds dinfo at its own info slots to dattrs only if a later-executed head can read them -- the last
 * executed head never does, no head of GGD_CHAIN_PARALLEL does; the first head of GGD_CHAIN_SEQUENTIAL (xyz) receives
 * 0.01 * (dattrs + dinfo).
 * Every ggd_decoder_* entry point has a *_chain form that takes the chain behind `stream`; the form without it is the
 * GGD_CHAIN_SEQUENTIAL_REVERSED call.  An unknown chain value returns GGD_E_INVALID.  The image sizes, ggd_decoder_zbuf_bytes
 * and ggd_decoder_wgrad_floats do not depend on the chain.
 */
typedef enum ggd_decoder_chain {
  GGD_CHAIN_SEQUENTIAL_REVERSED = 0,
  GGD_CHAIN_SEQUENTIAL = 1,
  GGD_CHAIN_PARALLEL = 2
} ggd_decoder_chain;
int ggd_decoder_pack_chain(ggd_ctx* ctx, void* stream, int32_t chain, const float* const* params40, void* packed,
                           void* packed_t);
int ggd_decoder_forward_chain(ggd_ctx* ctx, void* stream, int32_t chain, const float* feat, const float* pos, int32_t N,
                              const void* packed_weights, float* attrs);

/*
 * Fused decoder, TRAINING.  ggd_decoder_forward_train == ggd_decoder_forward that also keeps the hidden layers'
 * pre-activations: zbuf[5 heads][3 layers][ceil(N/16) blocks][16 points x 128] bf16 (ggd_decoder_zbuf_bytes(N); opaque:
 * inside a 4 KB block the values sit in the register order of the kernels, see csrc/ggd_mlp.hip).
 * ggd_decoder_backward: given dattrs[N,16] (gradient w.r.t. the attrs rows) it back-propagates through the 5 heads
 * (last first) with the TRANSPOSED weight image packed_t (ggd_decoder_packed_t_bytes(); built by
 * fused_decoder.pack_weights_t) and writes
 *   dzbuf (same size and layout as zbuf)  gradient at every hidden pre-activation
 *   dout  [5][N][4]      fp32  gradient at every head's raw output (columns >= the head's width are zero)
 *   dfeat [N,32]         fp32  gradient w.r.t. the plane features (sum over the 5 heads)
 *   dinfo [N,16]         fp32  scratch (gradient carried between heads through the chained inputs)
 * The weight / bias gradients are reductions over the N points of dz_l^T h_{l-1}; the caller forms them as split-K
 * GEMMs from dzbuf / dout and the activations (fused_decoder.FusedDecoderFn).
 */
size_t ggd_decoder_zbuf_bytes(int32_t N);
size_t ggd_decoder_packed_t_bytes(void);
int ggd_decoder_forward_train(ggd_ctx* ctx, void* stream, const float* feat, const float* pos, int32_t N,
                              const void* packed_weights, float* attrs, void* zbuf);
int ggd_decoder_backward(ggd_ctx* ctx, void* stream, int32_t N, const void* packed_t, const float* attrs,
                         const float* dattrs, const void* zbuf, void* dzbuf, float* dout, float* dfeat, float* dinfo);
int ggd_decoder_forward_train_chain(ggd_ctx* ctx, void* stream, int32_t chain, const float* feat, const float* pos, int32_t N,
                                    const void* packed_weights, float* attrs, void* zbuf);
int ggd_decoder_backward_chain(ggd_ctx* ctx, void* stream, int32_t chain, int32_t N, const void* packed_t, const float* attrs,
                               const float* dattrs, const void* zbuf, void* dzbuf, float* dout, float* dfeat, float* dinfo);

/*
 * Weight / bias gradients of the fused decoder: split-K MFMA GEMMs over the points, operands transposed through LDS
 * (ds_read_b64_tr_b16), gelu(z) recomputed on the fly.  ACCUMULATES (fp32 atomics) into wgrad, which the caller
 * zero-initialises: ggd_decoder_wgrad_floats() floats = 5 heads x
 *   { dW1[128][64] db1[128] dW2[128][128] db2[128] dW3[128][128] db3[128] dW4[16][128] db4[16] }
 * (dW1 columns: 32 plane features, 3 position, then the earlier heads' outputs; columns / rows past the layer's real
 * width are padding).  feat / pos / attrs as in ggd_decoder_forward_train, zbuf from it, dzbuf / dout from
 * ggd_decoder_backward.
 */
size_t ggd_decoder_wgrad_floats(void);
int ggd_decoder_wgrad(ggd_ctx* ctx, void* stream, int32_t N, const void* zbuf, const void* dzbuf, const float* dout,
                      const float* feat, const float* pos, const float* attrs, float* wgrad);
int ggd_decoder_wgrad_chain(ggd_ctx* ctx, void* stream, int32_t chain, int32_t N, const void* zbuf, const void* dzbuf,
                            const float* dout, const float* feat, const float* pos, const float* attrs, float* wgrad);

/*
 * Fused image losses of the decoder training step and their gradient (main/train_pano2gaussian_decoder.py:246-261
 * without the external-network terms):
 *   loss = w[0]*L1 + w[1]*L2 + w[2]*(1 - SSIM) + w[3]*Sobel
 * with l1_loss / l2_loss / ssim of gaussian_splatting/utils/loss_utils.py:17-63 and sobel_loss of
 * main/loss_utils/sobel_loss.py:19-30.  image, target: device [3,H,W] fp32.  weights4: HOST array of 4 floats.
 * terms5 (device, 5 floats): L1, L2, 1 - SSIM, Sobel, weighted total.  grad_image (device [3,H,W]) = dloss/dimage.
 * tmp: device scratch of ggd_image_loss_tmp_bytes(W, H) bytes.  Three kernel launches, no host sync.
 */
size_t ggd_image_loss_tmp_bytes(int32_t W, int32_t H);
int ggd_image_loss(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* image, const float* target,
                   const float* weights4, float* terms5, float* grad_image, void* tmp, size_t tmp_bytes);

/*
 * The same losses with --apply_mask_to_rendering (main/train_pano2gaussian_decoder.py:237-241): mask (device
 * [mask_h, mask_w] fp32, H % mask_h == 0 and W % mask_w == 0, otherwise GGD_E_INVALID) is upsampled bilinearly by the
 * integer factors H / mask_h, W / mask_w (torch.nn.functional.interpolate, align_corners=False) to m, and image and target
 * are composited onto white, x' = (x*m + 1) - m, before every term; terms5 are those of the composited pair and
 * grad_image = m * dloss/dimage'.  No gradient for target or mask.  Still three launches and the same tmp; neither the
 * full-resolution mask nor the composited images are materialised.
 * ggd_mask_composite: the composite as an operator of its own over src [channels,H,W] (for consumers that need the
 * composited image itself): backward == 0: dst = (src*m + 1) - m; backward != 0: dst = src*m (src is then d/d dst).
 */
int ggd_image_loss_masked(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* image, const float* target,
                          const float* mask, int32_t mask_w, int32_t mask_h, const float* weights4, float* terms5,
                          float* grad_image, void* tmp, size_t tmp_bytes);
int ggd_mask_composite(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, int32_t channels, const float* src,
                       const float* mask, int32_t mask_w, int32_t mask_h, int32_t backward, float* dst);

/*
 * Geometry loss: the rasterizer's depth D = sum alpha_i T_i z_i and alpha A = 1 - final T (device [H,W] fp32, the aux maps
 * of ggd_forward_aux) against the teacher's depth t and weights w (device [th,tw] fp32; H % th == 0 and W % tw == 0,
 * otherwise GGD_E_INVALID), and its gradient.  With xl = (2 (j + 0.5) / tw - 1) tanfovx, yl = (2 (i + 0.5) / th - 1) tanfovy:
 *   z[i,j] = t[i,j] / sqrt(1 + xl^2 + yl^2) if ray_depth != 0 (t is a distance along a unit ray), else t[i,j];   p = w z;
 *   m = up(w), q = up(p): the bilinear upsample of ggd_image_loss_masked by the integer factors H / th, W / tw;
 *   r_m = A - m,  r_d = m D - A q;   L_mask = mean |r_m|,  L_depth = mean |r_d|  (means over H W);
 *   total = weights2[0] L_mask + weights2[1] L_depth.
 * weights2: HOST array of 2 floats.  terms3 (device, 3 floats): L_mask, L_depth, total.  grad_depth, grad_alpha (device
 * [H,W]): dtotal/dD = weights2[1] sgn(r_d) m / (H W), dtotal/dA = (weights2[0] sgn(r_m) - weights2[1] sgn(r_d) q) / (H W),
 * sgn(0) = 0.  No gradient for the teacher's maps.  Precondition (not checked): t is finite.
 * tmp: device scratch of ggd_geometry_loss_tmp_bytes(W, H) bytes.  Two kernel launches, no host sync, no float atomics:
 * terms and gradients are bit-identical from run to run.
 */
size_t ggd_geometry_loss_tmp_bytes(int32_t W, int32_t H);
int ggd_geometry_loss(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* depth, const float* alpha,
                      const float* teacher_depth, const float* teacher_weights, int32_t tw, int32_t th, float tanfovx,
                      float tanfovy, int32_t ray_depth, const float* weights2, float* terms3, float* grad_depth,
                      float* grad_alpha, void* tmp, size_t tmp_bytes);

/*
 * Per-Gaussian view-space normals (csrc/ggd_normals.hip): a splat's shortest axis, turned towards the camera.  All arrays DEVICE
 * fp32: rotations [P,4] (w,x,y,z; 16-byte aligned), scales [P,3], means3D [P,3], viewmatrix [16] in the rasterizer's layout
 * (p_view = p . V[:3,:3] + V[3,:3], V[a][c] = viewmatrix[4a + c]).  Per row:
 *   raw == 0: q = the quaternion as given (not re-normalised);  raw != 0: q = rotation / max(|rotation|, 1e-12), the rule of the
 *             rasterizer's fused-activation prologue (a zero quaternion stays zero: R = I), and scales are the raw log-scales
 *             (exp is monotonic: the same argmin);
 *   k = argmin_j scales[j], ties to the lowest index;   n_w = column k of R(q), R the matrix the rasterizer builds Sigma = R S S R^T from;
 *   n_v = n_w . V[:3,:3];   p_v = the view-space mean;   normals[row] = -n_v if n_v . p_v > 0, else n_v   (so n . p_v <= 0).
 * ggd_gaussian_normals_backward: dL_drotations [P,4] (16-byte aligned) = J^T dL_dnormals, J the derivative of column k of R in
 * (w,x,y,z) through V and the sign, and through the normalisation when raw.  Scales, means and the view matrix get no gradient:
 * the argmin and the facing sign are decisions.  One launch each, one thread per Gaussian; no atomics, no scratch, no host wait.
 * P == 0 is legal and launches nothing; P < 0, a NULL or a misaligned pointer: GGD_E_INVALID, nothing launched.
 */
int ggd_gaussian_normals(ggd_ctx* ctx, void* stream, int32_t P, const float* rotations, const float* scales,
                         const float* means3D, const float* viewmatrix, int32_t raw, float* normals);
int ggd_gaussian_normals_backward(ggd_ctx* ctx, void* stream, int32_t P, const float* rotations, const float* scales,
                                  const float* means3D, const float* viewmatrix, int32_t raw, const float* dL_dnormals,
                                  float* dL_drotations);

/*
 * Normal-consistency loss (2DGS / gsplat / PGSR): the blended normal map N_r = sum alpha_i T_i n_i (device [3,H,W] fp32,
 * unnormalised: a feature map of ggd_forward_features over ggd_gaussian_normals) against the normals of the surface that the
 * depth map describes, and its gradient.  depth = sum alpha_i T_i z_i and alpha A (device [H,W], the aux maps).  Pixel (i, j) has
 * x_j = (2 (j + 0.5) / W - 1) tanfovx, y_i = (2 (i + 0.5) / H - 1) tanfovy (the rasterizer's pixel centres, as ggd_geometry_loss);
 *   ok(p) = A(p) > alpha_min;   D = depth / A;   P = (x_j D, y_i D, D);
 *   at an interior pixel whose own ok and its four axis neighbours' ok hold:
 *     dU = P(i, j+1) - P(i, j-1),  dV = P(i+1, j) - P(i-1, j),  c = dV x dU  (faces the camera: (0, 0, -1) on a fronto-parallel plane),
 *     N_s = c / |c| (0 if |c| = 0),  e = A - N_r . N_s;
 *   everywhere else e = 0 and N_s = 0;   L = sum e / (H W).
 * term (device, 1 float) = L.  grad_normals [3,H,W], grad_depth, grad_alpha [H,W]: the exact derivative of L as stated -- nothing is
 * detached, the path through D into the neighbours' N_s included.  surface_normals: NULL, or [3,H,W] that receives N_s.
 * tmp: device scratch of ggd_normal_loss_tmp_bytes(W, H) bytes.  Two kernel launches (the per-pixel pass; the gather of the
 * transposed stencil, whose first workgroup also adds the per-workgroup partial sums), no host sync, no float atomics: term and
 * gradients are bit-identical from run to run.  GGD_E_INVALID, nothing launched: W or H <= 0, a NULL pointer other than
 * surface_normals, alpha_min < 0 (or NaN), a tmp that is too small.
 */
size_t ggd_normal_loss_tmp_bytes(int32_t W, int32_t H);
int ggd_normal_loss(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* normals, const float* depth,
                    const float* alpha, float tanfovx, float tanfovy, float alpha_min, float* term, float* grad_normals,
                    float* grad_depth, float* grad_alpha, float* surface_normals /* or NULL */, void* tmp, size_t tmp_bytes);

/*
 * Exact 3-nearest-neighbour search: the `distCUDA2` of the simple_knn module that gaussian_splatting/scene/gaussian_model.py
 * imports (:20) to seed the scales of a new model (:132, :160).  points: DEVICE float32 [P][3], 4 <= P <= ggd_knn_max_points()
 * (2^26; fewer than 4 points have no three neighbours: GGD_E_INVALID).  For every point i, over all j != i (a different INDEX:
 * coincident points count, distance 0), d = (dx*dx + dy*dy) + dz*dz in fp32 without contraction, the three smallest kept
 * ascending b0 <= b1 <= b2:
 *   mean_dist2[i] = ((b0 + b1) + b2) / 3.0f     dist2[i] = {b0, b1, b2}     idx[i] = rows of the three points
 * (each output may be NULL; all are indexed by the ORIGINAL row order; among equal distances any candidate may be named).
 * The values are exact: bit-identical to a brute force that evaluates the same expression, from run to run and under any
 * permutation of the rows.  Rows with non-finite coordinates get unspecified values; the call still terminates.
 * examined: NULL, or a DEVICE counter the call ADDS the number of evaluated candidate points to (summed over all queries;
 * a separately compiled kernel instance, the plain call pays nothing) -- a work measure: a small multiple of
 * P * ggd_knn_leaf_size() on well-spread input, and just under P * ggd_knn_leaf_size() for P copies of one point.
 * tmp: ggd_knn_tmp_bytes(P) bytes of device scratch, 16-byte aligned (about 22 bytes per point).  No allocation, no host
 * synchronisation, no float atomics inside the call.
 * ggd_knn3_stage (timing aid, scripts/knn_timing.py): runs ONE stage (0 box, 1 Morton codes, 2 sort, 3 leaves, 4 search) on
 * a tmp that holds the results of the earlier stages of a previous call on the same points.
 */
size_t ggd_knn_tmp_bytes(int32_t P);
int32_t ggd_knn_leaf_size(void);
int32_t ggd_knn_max_points(void);
int ggd_knn3(ggd_ctx* ctx, void* stream, const float* points, int32_t P, float* mean_dist2 /* [P] or NULL */,
             float* dist2 /* [P,3] ascending, or NULL */, int32_t* idx /* [P,3] or NULL */,
             unsigned long long* examined /* device counter or NULL */, void* tmp, size_t tmp_bytes);
int ggd_knn3_stage(ggd_ctx* ctx, void* stream, const float* points, int32_t P, float* mean_dist2, float* dist2, int32_t* idx,
                   unsigned long long* examined, void* tmp, size_t tmp_bytes, int32_t stage);

/*
 * Adaptive density control of a fitted scene: the statistics lines and densify_and_prune / prune_points of
 * gaussian_splatting/scene/gaussian_model.py (:453-546, train.py:115-120) as streaming passes (csrc/ggd_densify.hip).
 * All arrays are DEVICE float32 unless stated; P <= 2^26.
 *
 * ggd_densify_stats: one launch, in place, no host wait.  A row is visible when filter[i] != 0 (filter: uint8 [P]) or, without
 * a filter, when radii[i] > 0 (radii: int32 [P]); at least one of the two is given.  On visible rows
 *   accum[i] += sqrt(gx*gx + gy*gy) (grad_means2D: [P][3])    denom[i] += 1    max_radii2D[i] = max(max_radii2D[i], (float)radii[i])
 * (the last line only when max_radii2D is given, which needs radii); other rows are not touched.
 *
 * ggd_densify_plan: per row, g = accum / denom (0/0 = 0), s = exp(scaling [P][3]), smax = max s,
 *   hot = g >= max_grad   C = hot && smax <= split_threshold   S = hot && smax > split_threshold
 *   low = sigmoid(opacity) < min_opacity   big(x) = use_world_size && x > world_size
 *   prune_self = low || big(smax)   prune_child = low || big(exp(log(smax / 1.6)))
 * and the rows of the result, each segment in source order: originals with !S && !prune_self | raw copies of the rows with
 * C && !prune_self | first children of the rows with S && !prune_child | their second children -- the final state of the
 * reference's clone, split, prune sequence (its screen-size test never fires: max_radii2D is zero by then).  max_grad > 0
 * (GGD_E_INVALID otherwise: a clone's zero statistic would satisfy the split test).  Three launches (classify + reduce, block
 * sums, source map -- every dependency is a kernel boundary, nothing waits on another workgroup), then ONE read-back, for which
 * the call waits on `stream`: counts4 (HOST) = {originals kept, clones, split parents kept, new row count}.
 * ggd_prune_plan: the same with one segment, the rows with mask[i] == 0 (mask: uint8 [P]).
 * tmp: ggd_densify_tmp_bytes(P) bytes of device scratch, 16-byte aligned (about 9 bytes per row); it carries the plan to
 * ggd_densify_emit.  No allocation inside.
 *
 * ggd_densify_emit: one gather launch, one thread per output float, over the six parameter groups in optimizer order --
 * xyz [3], f_dc [3], f_rest [3 (M - 1)], opacity [1], scaling [3], rotation [4] floats per row -- and their Adam moments.
 * in18 / out18: HOST tables of 18 device pointers, [3 g + 0] the group's parameter, [3 g + 1] exp_avg, [3 g + 2] exp_avg_sq
 * (inputs P rows, outputs new_P rows; a group's four moment pointers may all be NULL: no optimizer state yet; f_rest is
 * ignored when M == 1).  Originals and clones are copied; a child (c = 0, 1) of row i gets
 *   xyz = R(rotation_i / |rotation_i|) (s_i * noise[c][i]) + xyz_i     scaling = log(s_i / 1.6)     the rest copied
 * with noise [2][P][3] standard-normal numbers of the caller (may be NULL for a plan without children).  Moments are copied
 * for kept originals and zero for every new row.  new_P is counts4[3] of the plan in tmp; new_P == 0 launches nothing.
 * ggd_densify_gather: out[r] = in[parent row of r] for any other [P][width] float array (1 <= width <= 64) through the same
 * plan, copies only -- the statistics arrays of prune_points.
 */
size_t ggd_densify_tmp_bytes(int32_t P);
int ggd_densify_stats(ggd_ctx* ctx, void* stream, int32_t P, const float* grad_means2D, const int32_t* radii /* or NULL */,
                      const uint8_t* filter /* or NULL */, float* accum, float* denom, float* max_radii2D /* or NULL */);
int ggd_densify_plan(ggd_ctx* ctx, void* stream, int32_t P, const float* accum, const float* denom, const float* scaling,
                     const float* opacity, float max_grad, float split_threshold, float min_opacity, int32_t use_world_size,
                     float world_size, void* tmp, size_t tmp_bytes, int64_t* counts4 /* host */);
int ggd_prune_plan(ggd_ctx* ctx, void* stream, int32_t P, const uint8_t* mask, void* tmp, size_t tmp_bytes,
                   int64_t* counts4 /* host */);
int ggd_densify_emit(ggd_ctx* ctx, void* stream, int32_t P, int32_t new_P, int32_t M, const float* const* in18,
                     float* const* out18, const float* noise /* [2][P][3] or NULL */, const void* tmp, size_t tmp_bytes);

int ggd_densify_gather(ggd_ctx* ctx, void* stream, int32_t P, int32_t new_P, int32_t width, const float* in, float* out,
                       const void* tmp, size_t tmp_bytes);

/*
 * Density control under a fixed row budget, "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024):
 * its compute_relocation op, relocate_gs, add_new_gs and the per-iteration position noise (csrc/ggd_mcmc.hip), restated from
 * the published source.  All arrays are DEVICE memory, float32 unless stated; P <= 2^26.  No call waits for the device, reads
 * anything back or allocates.
 *
 * Relocation values of a row with raw opacity x (o = sigmoid(x)) and ratio N in 1..51:
 *   o' = 1 - (1 - o)^(1/N)     D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1)     s' = s o / D
 * evaluated in fp64 from sp = softplus(x): o' = -expm1(-sp / N), new raw opacity = log(expm1(sp / N)) with o' clamped to
 * [0.005, 1 - 2^-23], new raw scale = raw scale + log(o / D).
 *
 * Sampling plan: weight w_i = max(1, round(sigmoid(x_i) * 2^20)) (uint32) on alive rows, 0 on dead ones; W = sum w (64 bits).
 * A destination with draw d (int64, its low 32 bits are used) picks tau = floor(d W / 2^32) and the source is the row whose
 * interval [C_i, C_i + w_i) of the exclusive prefix sum C holds tau; count[source] += 1 and N(source) = min(51, 1 + count).
 * Integer arithmetic only: the plan is a pure function of the weights and the draws.  W == 0 or no destination: nothing moves.
 *
 * ggd_mcmc_relocate: in place on io18 (the table of ggd_densify_emit: [3 g + 0] parameter, [3 g + 1] exp_avg, [3 g + 2]
 * exp_avg_sq of group g; P rows each; a group's moments may both be NULL).  Destinations are the dead rows: dead_mask[i] != 0
 * (uint8 [P]) or, with dead_mask NULL, sigmoid(x_i) <= 0.005.  draws: int64 [P], entry j is read when row j is dead.  Five
 * launches: weights, tile prefixes, sample, values (into tmp), then: a destination copies its source's xyz, f_dc, f_rest and
 * rotation and takes the source's new raw opacity and scales; a sampled source takes the same values and both Adam moments of
 * its row become 0 in all six groups; a destination's moments and every other row stay as they are.
 * ggd_mcmc_add_plan: the same plan with every row alive and num destinations (draws: int64 [num]), launches 1 - 4.
 * ggd_mcmc_add_emit: one launch that writes out18 (P + num rows) from in18 (P rows) and the plan in tmp: old rows copied, sampled
 * sources with their new raw opacity and scales and zero moments, row P + k a copy of source s_k with the new values and zero
 * moments.  num > 0 in both.
 * tmp: ggd_mcmc_tmp_bytes(P, n_dest) bytes, 16-byte aligned; n_dest = P for ggd_mcmc_relocate, num for the add pair.  It holds,
 * in this order and each aligned to 256 bytes: uint32 weights [T], uint32 in-tile prefixes [T] (T = P rounded up to 2048),
 * uint64 tile prefixes [T / 2048 + 1] (the last is W), uint32 counts [P], uint32 sources [n_dest] (0xFFFFFFFF: no destination),
 * float new values [P][4].
 *
 * ggd_mcmc_noise: one launch, xyz += Sigma (((xi * gate) * noise_lr) * xyz_lr) per row, Sigma = R S^2 R^T with R of the raw
 * quaternion normalised as the rasterizer does, S = exp(raw scale), gate = 1 / (1 + exp(-100 ((1 - o) - 0.995))) and
 * 1 - o = sigmoid(-x); noise: [P][3] standard-normal numbers of the caller.  rotation must be 16-byte aligned.
 *
 * ggd_compute_relocation: the op on activated values: new_opacities [n] = o', new_scales [n][3] = s' (no clamp), ratios int32 [n]
 * clamped to 1..51.
 */
size_t ggd_mcmc_tmp_bytes(int32_t P, int32_t n_dest);
int ggd_mcmc_relocate(ggd_ctx* ctx, void* stream, int32_t P, int32_t M, float* const* io18, const uint8_t* dead_mask /* or NULL */,
                      const int64_t* draws, void* tmp, size_t tmp_bytes);
int ggd_mcmc_add_plan(ggd_ctx* ctx, void* stream, int32_t P, int32_t num, const float* opacity, const float* scaling,
                      const int64_t* draws, void* tmp, size_t tmp_bytes);
int ggd_mcmc_add_emit(ggd_ctx* ctx, void* stream, int32_t P, int32_t num, int32_t M, const float* const* in18,
                      float* const* out18, const void* tmp, size_t tmp_bytes);
int ggd_mcmc_noise(ggd_ctx* ctx, void* stream, int32_t P, float* xyz, const float* scaling, const float* rotation,
                   const float* opacity, const float* noise, float noise_lr, float xyz_lr);
int ggd_compute_relocation(ggd_ctx* ctx, void* stream, int32_t n, const float* opacities, const float* scales,
                           const int32_t* ratios, float* new_opacities, float* new_scales);

/*
 * Sparse Adam of the fitting loop (csrc/ggd_adam.hip): the published adamUpdate rule of the accelerated 3DGS rasterizer
 * (SparseGaussianAdam) over up to 8 parameter groups in ONE launch, in place, with no host wait, no allocation and no
 * device-side table (`groups` is HOST memory and travels by value in the kernel arguments).
 * A group is four DEVICE float32 arrays [N][width]; grad == NULL or width == 0 skips the group.  Exactly one of visible
 * (uint8 [N]: row i is updated when visible[i] != 0) and radii (int32 [N]: when radii[i] > 0, as in ggd_densify_stats) is
 * given.  Per element of an updated row, in fp32, every operation rounded on its own, in this order:
 *   m' = (b1 * m) + ((1.0f - b1) * g)     v' = (b2 * v) + (((1.0f - b2) * g) * g)     p' = p + (((-lr) * m') / (sqrtf(v') + eps))
 * (no bias correction, no step counter).  For a row that is not updated no byte of param, grad or the moments is loaded and
 * none is stored: a NaN there is never seen.  Arrays whose four base pointers are congruent modulo 16 move as 16-byte
 * accesses (any common offset from a 16-byte boundary will do); other groups are run one float at a time.
 * GGD_E_INVALID, nothing launched: NULL ctx or table; N < 0 or N > 2^26; n_groups outside 1..8; both or neither of visible /
 * radii; width < 0 or N * width >= 2^31; a group that is not skipped with a NULL param or moment, or a pointer that is not
 * 4-byte aligned.  N == 0 and a table of skipped groups are legal and launch nothing.
 */
typedef struct {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;   /* [N][width] float32 each; grad NULL = skip group */
  int32_t width;                                                        /* floats per row; 0 = skip group */
  float lr, eps;
} ggd_adam_group;
int ggd_adam_sparse(ggd_ctx* ctx, void* stream, int32_t N, int32_t n_groups, const ggd_adam_group* groups /* host memory */,
                    const uint8_t* visible /* [N] or NULL */, const int32_t* radii /* [N] or NULL */,
                    float beta1, float beta2);

/* ggd_decoder_backward + ggd_decoder_wgrad over point chunks of `chunk` points, each chunk's weight-gradient kernel launched
 * right behind its backward kernel so that it reads dz / z from the Infinity Cache.  chunk <= 0 or chunk > N: one chunk;
 * otherwise `chunk` is ROUNDED UP to a multiple of 256 points (one batch of a backward workgroup = four weight-gradient
 * stages), so that every chunk but the last starts and ends on the boundaries of the 16-point blocks of zbuf / dzbuf, of
 * the 32-point slabs and of the 64-point stages: chunk = 1 runs 256 points per launch pair, chunk = 300 runs 512.  dfeat,
 * dinfo, dout and dzbuf do not depend on `chunk` (bit for bit); wgrad is summed by float atomics in either form.
 * ggd_decoder_backward_wgrad_hl rounds `chunk` the same way. */
int ggd_decoder_backward_wgrad(ggd_ctx* ctx, void* stream, int32_t N, int32_t chunk, const void* packed_t,
                               const float* attrs, const float* dattrs, const void* zbuf, void* dzbuf, float* dout,
                               float* dfeat, float* dinfo, const float* feat, const float* pos, float* wgrad);
int ggd_decoder_backward_wgrad_chain(ggd_ctx* ctx, void* stream, int32_t chain, int32_t N, int32_t chunk, const void* packed_t,
                                     const float* attrs, const float* dattrs, const void* zbuf, void* dzbuf, float* dout,
                                     float* dfeat, float* dinfo, const float* feat, const float* pos, float* wgrad);

/*
 * The fused decoder at REFERENCE PRECISION (the reference trains its decoder in fp32, main/decoder_models/base_decoder.py:8-27):
 * same kernels' structure on the bf16 matrix cores with every fp32 operand split into two bf16 numbers (x = hi + lo) and
 * every product evaluated as W_hi x_hi + W_hi x_lo + W_lo x_hi with fp32 accumulation (csrc/ggd_mlp_hl.inc), in the forward,
 * the backward and the weight gradients (outputs within 1e-5 of an fp32 evaluation).
 * The weight images have their own format (hi and lo image per layer): ggd_decoder_pack_hl builds both from the 40
 * parameter tensors (see ggd_decoder_pack).  zbuf: ggd_decoder_zbuf_bytes(N) as in the bf16 form (fp16 values in both); dzbuf:
 * ONE fp16 plane, every (head, 32-point slab) scaled by its own power of two, ggd_decoder_dzbuf_hl_bytes(N) =
 * ggd_decoder_zbuf_bytes(N); dout / dfeat / dinfo / wgrad as in the bf16 entry points (ggd_decoder_forward_hl with zbuf == NULL is the inference form).
 */
size_t ggd_decoder_packed_hl_bytes(void);
size_t ggd_decoder_dzbuf_hl_bytes(int32_t N);
size_t ggd_decoder_packed_t_hl_bytes(void);
int ggd_decoder_pack_hl(ggd_ctx* ctx, void* stream, const float* const* params40, void* packed_hl, void* packed_t_hl);
int ggd_decoder_forward_hl(ggd_ctx* ctx, void* stream, const float* feat, const float* pos, int32_t N,
                           const void* packed_hl, float* attrs, void* zbuf);
int ggd_decoder_backward_wgrad_hl(ggd_ctx* ctx, void* stream, int32_t N, int32_t chunk, const void* packed_t_hl,
                                  const float* attrs, const float* dattrs, const void* zbuf, void* dzbuf, float* dout,
                                  float* dfeat, float* dinfo, const float* feat, const float* pos, float* wgrad);
int ggd_decoder_pack_hl_chain(ggd_ctx* ctx, void* stream, int32_t chain, const float* const* params40, void* packed_hl,
                              void* packed_t_hl);
int ggd_decoder_forward_hl_chain(ggd_ctx* ctx, void* stream, int32_t chain, const float* feat, const float* pos, int32_t N,
                                 const void* packed_hl, float* attrs, void* zbuf);
int ggd_decoder_backward_wgrad_hl_chain(ggd_ctx* ctx, void* stream, int32_t chain, int32_t N, int32_t chunk,
                                        const void* packed_t_hl, const float* attrs, const float* dattrs, const void* zbuf,
                                        void* dzbuf, float* dout, float* dfeat, float* dinfo, const float* feat,
                                        const float* pos, float* wgrad);

/*
 * The teacher's density field sampled on the device: what G.sample_mixed evaluates every iteration of the reference's
 * target loader (main/decoder_utils/target_dataloader.py:134-169) -- sample_from_planes, then OSGDecoder (mean over the
 * three planes, 32 -> 64 softplus -> 1 + 32; eg3d / PanoHead training/triplane.py) -- in ONE launch and with no intermediate
 * tensor (csrc/ggd_density.hip).  Per point:
 *   f = the 32 features of ggd_planes_gather (same planes, C, D, H, W, axes, box_warp; no modulation)
 *   h = softplus(w1 f + b1)            softplus(z) = z > 20 ? z : log1p(exp(z))
 *   sigma = w2[0] . h + b2[0];   rgb = act(w2[1:33] h + b2[1:33])
 * w1 [64][32], b1 [64], w2 [33][64], b2 [33]: the EFFECTIVE fp32 weights (FullyConnectedLayer's weight * weight_gain and
 * bias * bias_gain already applied).  rgb_act: 0 sigmoid(x) * 1.002 - 0.001 (EG3D, PanoHead "sigmoid"), 1 leaky_relu(x, 0.2)
 * * sqrt(2) (PanoHead "lrelu"), 2 none.  rgb [N][32], or NULL: sigma only -- the 32 rgb rows are then never read or computed,
 * and sigma is bit-identical to that of a call with rgb.  C must be 32 (64 hidden units and 32 rgb channels are fixed):
 * anything else is GGD_E_INVALID.  All arithmetic is fp32; no atomics: results are bit-identical from run to run.  A point
 * with a non-finite coordinate has no taps on the planes that coordinate reaches (zero features there).
 *
 * ggd_density_points: explicit coordinates pos [N][3].
 * ggd_density_grid:   the n^3 samples of the reference's lattice (main/marching_cube/sample.py:5-26, create_samples), generated
 *   in registers; sigma [n^3] comes out flat in sample order = [x][y][z], z fastest -- what ggd_surface_sample reads.
 *   lattice 0: the reference's arithmetic, op for op in fp32: t_z = i mod n, t_y = fmod(float(i) / n, n), t_x = fmod((float(i)
 *   / n) / n, n) (un-floored: the y and x indices carry fractional parts and x, y reach past the box), coordinate =
 *   fl(fl(t * voxel) + origin) with voxel = (float)(cube_length / (n - 1)) and origin = (float)(-cube_length / 2), both formed
 *   in DOUBLE (hence the double argument).  lattice 1: the regular lattice (floored indices).  2 <= n <= 1024.
 * ggd_density_lattice: the coordinates themselves, pos [n^3][3] (the reference's use_marching_cubes = False branch keeps
 *   samples[sigmas > 10]); bit-identical to what ggd_density_grid samples.
 */
int ggd_density_points(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                       int32_t axes, float box_warp, const float* w1, const float* b1, const float* w2, const float* b2,
                       int32_t rgb_act, const float* pos, int32_t N, float* sigma, float* rgb /* NULL = skip */);
int ggd_density_grid(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                     int32_t axes, float box_warp, const float* w1, const float* b1, const float* w2, const float* b2,
                     int32_t rgb_act, int32_t n, double cube_length, int32_t lattice, float* sigma,
                     float* rgb /* NULL = skip */);
int ggd_density_lattice(ggd_ctx* ctx, void* stream, int32_t n, double cube_length, int32_t lattice, float* pos);

/*
 * The teacher's feature, depth and weight maps (csrc/ggd_teacher.hip): what ImportanceRenderer.forward and MipRayMarcher2 compute
 * per ray (PanoHead training/volumetric_rendering/renderer.py:100-323, ray_marcher.py:27-57; eg3d .../renderer.py:88-140) --
 * stratified coarse depths, the field above at the coarse samples, the march, importance resampling, the field at the fine
 * samples, the union ordered by depth, the second march -- in six launches, no host wait, scratch in the context's workspace.
 * Planes, weights and rgb_act as in ggd_density_points.  origins, dirs [M][3] (device).  Per ray, all fp32:
 *   coarse depth k   fl(coarse_table[k] + fl(u_coarse[k] * delta)),  delta = (float)((ray_end - ray_start) / (Nc - 1)) formed in
 *                    DOUBLE (hence the double arguments);  coarse_table: HOST pointer to the Nc values of
 *                    torch.linspace(ray_start, ray_end, Nc), copied into the launch's arguments
 *   coordinate       fl(o + fl(depth * d));   field: ggd_density_points at that coordinate, bit for bit
 *   crop (use_crop)  sigma = -1e3 where !(|x| <= lim && |z| <= lim),  lim = (float)crop_limit  (box_warp / 2 - triplane_crop,
 *                    formed by the caller in double)
 *   march            midpoints of depth, sigma and rgb; softplus(sigma_mid - 1); alpha = 1 - exp(-sigma_mid * width);
 *                    w = alpha * exclusive cumprod(1 - alpha + 1e-10)
 *   importance       max_pool1d(2, 1, pad 1), avg_pool1d(2, 1), + 0.01, both ends dropped, + 1e-5, normalised, cumulative sum with
 *                    a leading 0, searchsorted(right) of u_fine, the denom < 1e-5 -> 1 rule, linear interpolation in the mid-depths
 *   composite        features = sum w rgb_mid (+ 1 - sum w with white_back), weights = sum w, depth = sum(w depth_mid) / sum w,
 *                    NaN -> +inf, clamped to the minimum and maximum over every sample depth of the call (all rays)
 * The scans and sums along a ray accumulate in double in one fixed order and round once; no atomics: bit-identical from run to
 * run.  u_coarse [M][Nc], u_fine [M][Ni] (NULL with Ni = 0): the reference's two rand draws, in [0, 1).  4 <= Nc <= 64,
 * 0 <= Ni <= 64 (0: the coarse-only branch), finite ray_start < ray_end, M * (Nc + Ni) < 2^31; anything else, and anything
 * ggd_density_points refuses, is GGD_E_INVALID before anything is launched.
 * Outputs: features [M][32], depth [M], weights [M].  samples: NULL, or a 16-byte aligned block of M * (Nc + Ni) * 37 floats that
 * receives every stage's values, in this order: rgb coarse [M][Nc][32], rgb fine [M][Ni][32], sigma coarse [M][Nc], sigma fine
 * [M][Ni] (both after the crop), depths coarse [M][Nc], depths fine [M][Ni], coordinates coarse [M][Nc][3], fine [M][Ni][3].
 */
int ggd_teacher_render(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                       int32_t axes, float box_warp, const float* w1, const float* b1, const float* w2, const float* b2,
                       int32_t rgb_act, const float* origins, const float* dirs, int32_t M, double ray_start, double ray_end,
                       const float* coarse_table /* host */, int32_t Nc, int32_t Ni, const float* u_coarse, const float* u_fine,
                       int32_t use_crop, double crop_limit, int32_t white_back, float* features, float* depth, float* weights,
                       float* samples /* NULL = workspace */);

/*
 * The perceptual term (csrc/ggd_perceptual.hip): losses.PerceptualStandIn -- perc() of main/loss_utils/lpips.py:16-34 with a
 * VGG16-shaped trunk of 13 3x3 convolutions (padding 1, ReLU), 2x2 max pools behind convolutions 1, 3, 6, 9 and five taps behind
 * 1, 3, 6, 9, 12 -- as HIP kernels: the forward, sum over the taps of |n_img - n_tgt|^2 with n = x / (|x|_c + 1e-10) *
 * sqrt(lin_c / (H W)), and the gradient into the image.  The twelve convolutions behind the first run on MFMA.
 *   tier GGD_PERC_BF16: f16 operands forward (clamped to +-65504), bf16 operands backward, fp32 accumulation;
 *   tier GGD_PERC_FP32: split-bf16 operands (hi + lo, three MFMAs per product) in both directions.
 * desc (HOST struct, DEVICE pointers inside):
 *   image [B][3][H_in][W_in] fp32 in; x = mean over (H_in / H) x (W_in / W) blocks of scale[c] * image + shift[c] enters the trunk
 *   at H x W (both multiples of 16 and divisors of H_in, W_in); widths[13]: output channels, each a multiple of 32, <= 512
 *   (widths[0] <= 64);
 *   w0 [27][widths[0]] fp32, row (ky * 3 + kx) * 3 + ci; w0_t [9][widths[0]][3] fp32, W[co][ci][ky][kx] at [ky * 3 + kx][co][ci];
 *   bias[l] [widths[l]] fp32; lin[k] [width of tap k] fp32;
 *   w_fwd[l], w_bwd[l] (l = 1..12): the weight images in MFMA fragment order -- losses.pack_conv_weights of the layer's weights,
 *   and of the flipped, transposed weights; f16 / bf16 for GGD_PERC_BF16, bf16 hi and lo for GGD_PERC_FP32.
 * ggd_perceptual_loss: target [B][3][H_in][W_in] goes through the forward with the image as one batch of 2 B; loss (device, 1
 * float) = the sum over the batch; grad_image (device [B][3][H_in][W_in], or NULL: forward only) = dloss/dimage.  No gradient
 * for the target or the weights.  ggd_perceptual_features: features [B][F] = the rows of PerceptualStandIn.features (per tap
 * [C][H_k][W_k] flattened, taps concatenated).  tmp: ggd_perceptual_tmp_bytes(desc, images in the forward (2 B for the loss, B for
 * the features), with_grad) bytes of device scratch; 0 for a shape, width or tier the kernels do not take, which the entries
 * refuse with GGD_E_INVALID before anything is launched.  No host sync, no float atomics: bit-identical from run to run.
 */
#define GGD_PERC_CONVS 13
#define GGD_PERC_TAPS 5
enum { GGD_PERC_BF16 = 0, GGD_PERC_FP32 = 1 };
typedef struct ggd_perceptual_desc {
  int32_t tier;
  int32_t B;
  int32_t H_in, W_in;
  int32_t H, W;
  int32_t widths[GGD_PERC_CONVS];
  float scale[3], shift[3];
  const float* w0;
  const float* w0_t;
  const float* bias[GGD_PERC_CONVS];
  const void* w_fwd[GGD_PERC_CONVS];   /* [0] unused */
  const void* w_bwd[GGD_PERC_CONVS];   /* [0] unused */
  const float* lin[GGD_PERC_TAPS];
} ggd_perceptual_desc;
size_t ggd_perceptual_tmp_bytes(const ggd_perceptual_desc* desc, int32_t n_images, int32_t with_grad);
int ggd_perceptual_loss(ggd_ctx* ctx, void* stream, const ggd_perceptual_desc* desc, const float* image, const float* target,
                        float* loss, float* grad_image /* or NULL */, void* tmp, size_t tmp_bytes);
int ggd_perceptual_features(ggd_ctx* ctx, void* stream, const ggd_perceptual_desc* desc, const float* image, float* features,
                            void* tmp, size_t tmp_bytes);

/* Per-stage device time (ms, hipEvent pairs on `stream`) of the most recent forward_geometry / forward_render /
 * backward call when profiling is on.  Stage names: ggd_stage_name(i), i in [0, ggd_stage_count()). */
int ggd_set_profiling(ggd_ctx* ctx, int enabled);
int ggd_stage_count(void);
const char* ggd_stage_name(int stage);
int ggd_stage_times(ggd_ctx* ctx, float* ms_out /* host, ggd_stage_count() floats, <0 = not run */);

#ifdef __cplusplus
}
#endif
#endif /* GGD_RASTER_H */
