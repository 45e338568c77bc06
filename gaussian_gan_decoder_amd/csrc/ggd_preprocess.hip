// ggd_preprocess.hip -- stage a4 (per-Gaussian forward) and a12 (mark_visible) for gfx950.
//
// Replaces the per-Gaussian half of `_C.rasterize_gaussians` that the reference reaches through
// gaussian_splatting/gaussian_renderer/__init__.py:167-175 (source not in the reference tree; algorithm restated
// in SURVEY.md section 9.2).  One lane per Gaussian, 256-lane workgroups; every input array is read exactly once
// with per-lane vector loads over contiguous addresses (a wave covers 64 consecutive Gaussians = one contiguous
// 768 B / 1 KiB span per array), and the outputs the blend needs are packed into ONE 48-byte record per Gaussian
// (ggd_splat) so that the per-tile gather later touches a single 64 B-aligned-ish record instead of four arrays.
// HBM-bound: 56 B in (degree 0) + 56 B out per visible Gaussian, 56 B in + 8 B out per culled one.
#include "ggd_math.h"

namespace {
using namespace ggdm;

// SHVEC (more than the band-0 coefficient per channel, rows a multiple of 16 bytes: M = 4, 8, 12, 16): a visible Gaussian's
// 3 M coefficients are fetched as 3 M / 4 dwordx4 loads into registers instead of 3 M lone words -- each such load
// instruction touches 64 different rows whatever its width (1 M Gaussians, M = 16: preprocess 76 -> see DESIGN.md).
// FOLD (ggd_fold, single-call forward on the tile-binning path): the workgroup also (a) clears its share of the OTHER
// control block for the next frame, (b) adds the four digit counts of its kept depth keys to replica blockIdx % REPS of the
// depth sort's histograms (LDS histogram first; bins that stayed empty cost nothing), (c) stores {sum of tiles_touched, kept
// keys} of its 256 points for the offsets scan -- the sort's histogram launch and the scan's first step disappear.
// The body is ggd_preprocess_body.inc, shared with the anti-aliasing overload below.
template <bool SHVEC, bool FOLD>
__global__ __launch_bounds__(256) void preprocess_kernel(
    int P, int M, int deg, int W, int H, float tanfovx, float tanfovy, float fx, float fy, float mod, int prefiltered, int raw,
    const float* __restrict__ view, const float* __restrict__ proj, const float* __restrict__ campos_p,
    const float* __restrict__ means3D, const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ opacities, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, ggd_splat* __restrict__ splat, uint32_t* __restrict__ tiles_touched,
    uint8_t* __restrict__ clamped, int32_t* __restrict__ radii, uint32_t* __restrict__ depth_keys,
    uint2* __restrict__ rect, uint32_t* __restrict__ trap_flag, uint32_t* __restrict__ zero_ptr, int zero_words,
    ggd_fold fold) {
  constexpr bool AA = false;
#include "ggd_preprocess_body.inc"
}

// The same with the opacity-compensated 2D filter (ggd_params.antialiasing; AA_ must be true: an overload, so that the plain
// instances keep their names).  The record's opacity -- and with it thr, ex, ey -- is o_eff = o h, h = sqrt(max(2.5e-5,
// det0 / det1)), det0 / det1 the determinants of the EWA 2D covariance before / after the 0.3 px^2 dilation (Mip-Splatting).
// The conic, radius, rect, tiles_touched and depth key come from the dilated covariance, as in the plain kernel.
template <bool SHVEC, bool FOLD, bool AA_>
__global__ __launch_bounds__(256) void preprocess_kernel(
    int P, int M, int deg, int W, int H, float tanfovx, float tanfovy, float fx, float fy, float mod, int prefiltered, int raw,
    const float* __restrict__ view, const float* __restrict__ proj, const float* __restrict__ campos_p,
    const float* __restrict__ means3D, const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ opacities, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, ggd_splat* __restrict__ splat, uint32_t* __restrict__ tiles_touched,
    uint8_t* __restrict__ clamped, int32_t* __restrict__ radii, uint32_t* __restrict__ depth_keys,
    uint2* __restrict__ rect, uint32_t* __restrict__ trap_flag, uint32_t* __restrict__ zero_ptr, int zero_words,
    ggd_fold fold) {
  static_assert(AA_, "the plain kernel is the two-parameter template");
  constexpr bool AA = true;
#include "ggd_preprocess_body.inc"
}

__global__ __launch_bounds__(256) void mark_visible_kernel(int P, const float* __restrict__ means3D,
                                                           const float* __restrict__ view,
                                                           uint8_t* __restrict__ present) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float x = means3D[3 * (size_t)i], y = means3D[3 * (size_t)i + 1], z = means3D[3 * (size_t)i + 2];
  const float tz = view[2] * x + view[6] * y + view[10] * z + view[14];
  present[i] = (uint8_t)(tz > 0.2f);
}

}  // namespace

int ggd_launch_preprocess(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const float* means3D,
                          const float* shs, const float* colors_precomp, const float* opacities,
                          const float* scales, const float* rotations, const float* cov3D_precomp,
                          ggd_splat* splat, uint32_t* tiles_touched, uint8_t* clamped, int32_t* radii,
                          uint32_t* depth_keys, uint2* rect, uint32_t* trap_flag, uint32_t* zero_ptr, int zero_words,
                          const ggd_fold* fold) {
  if (prm.P == 0) return GGD_OK;
  const int grid = (prm.P + 255) / 256;
  const bool shvec = !colors_precomp && prm.M > 1 && prm.M <= 16 && ((3 * prm.M) & 3) == 0;
  const ggd_fold f = fold ? *fold : ggd_fold{};
  // focal lengths: wave-uniform correctly rounded divisions, done once here (same fp32 expression, same result)
  const float fx = (float)prm.width / (2.0f * prm.tanfovx), fy = (float)prm.height / (2.0f * prm.tanfovy);
#define GGD_PREPROCESS(...)                                                                                                 \
  hipLaunchKernelGGL((preprocess_kernel<__VA_ARGS__>), dim3(grid), dim3(256), 0, s, prm.P, prm.M, prm.sh_degree, prm.width,     \
                     prm.height, prm.tanfovx, prm.tanfovy, fx, fy, prm.scale_modifier, prm.prefiltered, prm.raw_attributes,          \
                     prm.viewmatrix, prm.projmatrix, prm.campos, means3D, shs, colors_precomp, opacities, scales, rotations, \
                     cov3D_precomp, splat, tiles_touched, clamped, radii, depth_keys, rect, trap_flag, zero_ptr,             \
                     zero_ptr ? zero_words : 0, f)
  if (prm.antialiasing) {
    if (fold) { if (shvec) GGD_PREPROCESS(true, true, true); else GGD_PREPROCESS(false, true, true); }
    else { if (shvec) GGD_PREPROCESS(true, false, true); else GGD_PREPROCESS(false, false, true); }
  } else {
    if (fold) { if (shvec) GGD_PREPROCESS(true, true); else GGD_PREPROCESS(false, true); }
    else { if (shvec) GGD_PREPROCESS(true, false); else GGD_PREPROCESS(false, false); }
  }
#undef GGD_PREPROCESS
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

int ggd_launch_mark_visible(ggd_ctx* ctx, hipStream_t s, int P, const float* means3D, const float* view,
                            uint8_t* present) {
  if (P == 0) return GGD_OK;
  hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, present);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
