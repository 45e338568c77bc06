// ggd_teacher.hip -- the teacher's feature, depth and weight maps: rays -> composited rgb features, depth, weight sum.
//
// What the reference does on every step with ImportanceRenderer.forward (PanoHead training/volumetric_rendering/renderer.py:
// 100-196, eg3d .../renderer.py:88-140: sample_stratified, run_model, the crop, sample_importance / sample_pdf, unify_samples) and
// MipRayMarcher2.run_forward (ray_marcher.py:27-57) in ~40 torch launches over [rays, samples, 35] tensors.  Here: six launches,
//   1  tr_coarse_kernel      coarse depths fl(t[k] + fl(u * delta)) and coordinates fl(o + fl(depth * d)), one sample per lane
//   2  density_kernel<., true>  the field at the coarse coordinates (ggd_density.hip, through its pos source, unchanged)
//   3  tr_importance_kernel  crop, march, the two pools, pdf, cdf, inversion -> fine depths and coordinates
//   4  density_kernel<., true>  the field at the fine coordinates
//   5  tr_composite_kernel   crop (written back), rank of the union by depth, march, the three sums; the ray's depth range
//   6  tr_clamp_kernel       minimum / maximum over the rays' ranges, depth clamped to it (the reference clamps to the range of
//                            every sample depth of the call) -- the reduction stays on the device, no host wait anywhere
// With Ni = 0 (the reference's coarse-only branch) launches 3 and 4 are left out.
//
// Layout of 3 and 5: ONE RAY PER WAVE64, four rays per workgroup; lane l holds sample l of the coarse set and sample l of the
// fine set (Nc, Ni <= 64).  Neighbours along the ray come from lane shifts, the products and sums along the ray are wave scans,
// the cdf and the bins sit in the wave's LDS for the per-lane binary search, and the union is ordered by counting: the rank of a
// sample is the number of the <= 128 depths in LDS that are smaller (as order-preserving integer keys, so the ranks are a
// permutation whatever the values; a tie goes to the smaller index -- two samples of one ray at one depth are one point with one
// field value, so the order of a tie shows nowhere).  The 32-channel composite has channel c on lanes c and 32 + c: each half walks
// one half of the ordered intervals front to back, one 128-byte rgb row per step, and the two partial sums are added.
//
// Arithmetic.  Every per-element operation is fp32 in the reference's order (-ffp-contract=off; the coarse depths and the
// coordinates use the rounding intrinsics).  The scans and sums along a ray (cumprod, the pdf's normaliser, cumsum, the three
// composite sums) accumulate in double and round once to fp32: torch's CPU cumprod / cumsum accumulate in double too, and a
// double sum of <= 127 fp32 terms rounds to the correctly rounded fp32 sum whatever its order, so no fp32 summation order has
// to be matched.  No atomics; one fixed order per sum: bit-identical from run to run.
#include "ggd_common.h"
#include "ggd_density_launch.h"

#include <cmath>

namespace {

constexpr int TR_MAX = 64;         // samples per set: one lane each
constexpr int TR_MIN_COARSE = 4;   // the importance stage drops both ends of the Nc - 1 weights and needs one left
constexpr int TR_RAYS = 4;         // rays (waves) per workgroup
constexpr int TR_RGB = 32;         // rgb channels (the field's)
constexpr float TR_CROPPED = -1e3f;

struct TrTable { float t[TR_MAX]; };   // torch.linspace(ray_start, ray_end, Nc), passed by value

// the sample block: [rays][samples] arrays, coarse and fine apart so that each field launch reads and writes contiguous rows
struct TrSamples { float *rgb_c, *rgb_f, *sigma_c, *sigma_f, *depth_c, *depth_f, *xyz_c, *xyz_f; };

__device__ __forceinline__ float tr_softplus(float z) { return z > 20.0f ? z : log1pf(expf(z)); }   // torch's (threshold 20)

__device__ __forceinline__ bool tr_outside(float x, float z, float lim) { return !(fabsf(x) <= lim && fabsf(z) <= lim); }

// alpha of the interval between two adjacent samples: 1 - exp(-softplus(sigma_mid - 1) * width), evaluated as -expm1(.).  The
// literal form loses up to half an ulp OF 1 per interval (alpha is ~1e-2), and how exp rounds there differs between
// implementations: summed over ~100 intervals that showed as 5e-7 on the weight sum, above what two evaluations may differ by.
__device__ __forceinline__ float tr_alpha(float t0, float s0, float t1, float s1) {
  const float width = t1 - t0;
  const float dens = tr_softplus((s0 + s1) / 2.0f - 1.0f);
  return -expm1f(-(dens * width));
}

// inclusive scans and the sum over the wave, in double, one fixed order
__device__ __forceinline__ double tr_scan_mul(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v = t * v;
  }
  return v;
}
__device__ __forceinline__ double tr_scan_add(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v = t + v;
  }
  return v;
}
__device__ __forceinline__ double tr_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// an integer that orders like the float (and orders NaNs too): the ranks below are a permutation for any input
__device__ __forceinline__ uint32_t tr_key(float t) {
  const uint32_t b = __float_as_uint(t);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void tr_coarse_kernel(TrTable tab, float delta, int Nc, int64_t total,
                                                        const float* __restrict__ origins, const float* __restrict__ dirs,
                                                        const float* __restrict__ u, float* __restrict__ depth,
                                                        float* __restrict__ xyz) {
  __shared__ float s_tab[TR_MAX];
  if (threadIdx.x < TR_MAX) s_tab[threadIdx.x] = tab.t[threadIdx.x];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t r = i / Nc;
  const int k = (int)(i - r * Nc);
  const float t = __fadd_rn(s_tab[k], __fmul_rn(u[i], delta));
  depth[i] = t;
#pragma unroll
  for (int a = 0; a < 3; ++a) xyz[3 * i + a] = __fadd_rn(origins[3 * r + a], __fmul_rn(t, dirs[3 * r + a]));
}

__global__ __launch_bounds__(64 * TR_RAYS) void tr_importance_kernel(int M, int Nc, int Ni, int use_crop, float lim,
                                                                    const float* __restrict__ origins,
                                                                    const float* __restrict__ dirs,
                                                                    const float* __restrict__ u_fine, TrSamples sm) {
  __shared__ float s_cdf[TR_RAYS][TR_MAX];
  __shared__ float s_bins[TR_RAYS][TR_MAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ray = blockIdx.x * TR_RAYS + wv;
  const bool live = ray < M;                       // a wave past the last ray computes ray M - 1 again and writes nothing
  const int64_t r = live ? ray : M - 1;
  const int Nm = Nc - 1, Ns = Nc - 3;              // intervals of the march; bins of the pdf (both ends dropped)

  const int64_t ci = r * Nc + (lane < Nc ? lane : Nm);
  const float t = sm.depth_c[ci];
  float s = sm.sigma_c[ci];
  if (use_crop && tr_outside(sm.xyz_c[3 * ci], sm.xyz_c[3 * ci + 2], lim)) s = TR_CROPPED;
  const float tn = __shfl_down(t, 1), sn = __shfl_down(s, 1);
  const bool iv = lane < Nm;
  const float alpha = iv ? tr_alpha(t, s, tn, sn) : 0.0f;
  const double incl = tr_scan_mul(iv ? (double)((1.0f - alpha) + 1e-10f) : 1.0, lane);
  double through = __shfl_up(incl, 1);
  if (lane == 0) through = 1.0;
  const float w = iv ? alpha * (float)through : -INFINITY;    // -inf: max_pool1d's padding at both ends

  float wp = __shfl_up(w, 1);
  if (lane == 0) wp = -INFINITY;
  const float mp = fmaxf(wp, w);                              // max_pool1d(2, 1, padding 1): Nc values on lanes 0 .. Nm
  const float ap = (mp + __shfl_down(mp, 1)) / 2.0f;          // avg_pool1d(2, 1): Nm values
  const float apn = __shfl_down(ap, 1);                       // both ends dropped: bin j takes ap[j + 1]
  const bool pv = lane < Ns;
  const float wt = pv ? (apn + 0.01f) + 1e-5f : 0.0f;
  const float norm = (float)tr_sum((double)wt);
  const float pdf = pv ? wt / norm : 0.0f;
  const double c = tr_scan_add((double)pdf, lane);
  if (lane == 0) s_cdf[wv][0] = 0.0f;
  if (pv) s_cdf[wv][lane + 1] = (float)c;                     // cdf[0 .. Ns]
  if (iv) s_bins[wv][lane] = 0.5f * (t + tn);                 // the mid-depths; bins[0 .. Ns] are read
  __syncthreads();

  if (lane < Ni) {
    const int64_t fi = r * Ni + lane;
    const float u = u_fine[fi];
    int lo = 0, hi = Ns + 1;                                  // searchsorted(right=True): the number of cdf values <= u
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_cdf[wv][mid] <= u) lo = mid + 1; else hi = mid;
    }
    const int below = lo > 0 ? lo - 1 : 0, above = lo < Ns ? lo : Ns;
    const float c0 = s_cdf[wv][below], c1 = s_cdf[wv][above], b0 = s_bins[wv][below], b1 = s_bins[wv][above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.0f;
    const float tf = b0 + (u - c0) / denom * (b1 - b0);
    if (live) {
      sm.depth_f[fi] = tf;
#pragma unroll
      for (int a = 0; a < 3; ++a) sm.xyz_f[3 * fi + a] = __fadd_rn(origins[3 * r + a], __fmul_rn(tf, dirs[3 * r + a]));
    }
  }
}

__global__ __launch_bounds__(64 * TR_RAYS) void tr_composite_kernel(int M, int Nc, int Ni, int use_crop, float lim, int white_back,
                                                                   TrSamples sm, float* __restrict__ features,
                                                                   float* __restrict__ depth, float* __restrict__ weights,
                                                                   float* __restrict__ range) {
  __shared__ uint32_t s_key[TR_RAYS][2 * TR_MAX];   // the union's depths as ordering keys, coarse first
  __shared__ float s_t[TR_RAYS][2 * TR_MAX];        // ordered depths
  __shared__ float s_s[TR_RAYS][2 * TR_MAX];        // ordered sigma
  __shared__ int s_i[TR_RAYS][2 * TR_MAX];          // ordered sample index (coarse k, fine Nc + k)
  __shared__ float s_w[TR_RAYS][2 * TR_MAX];        // weight of the interval [p, p + 1]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ray = blockIdx.x * TR_RAYS + wv;
  const bool live = ray < M;
  const int64_t r = live ? ray : M - 1;
  const int n = Nc + Ni, nm = n - 1;

  // ---- the lane's coarse and fine sample; the crop is written back so that the caller's sigma is the marched one ------------
  float t0 = 0.0f, s0 = 0.0f, t1 = 0.0f, s1 = 0.0f;
  if (lane < Nc) {
    const int64_t i = r * Nc + lane;
    t0 = sm.depth_c[i]; s0 = sm.sigma_c[i];
    if (use_crop && tr_outside(sm.xyz_c[3 * i], sm.xyz_c[3 * i + 2], lim)) {
      s0 = TR_CROPPED;
      if (live) sm.sigma_c[i] = s0;
    }
    s_key[wv][lane] = tr_key(t0);
  }
  if (lane < Ni) {
    const int64_t i = r * Ni + lane;
    t1 = sm.depth_f[i]; s1 = sm.sigma_f[i];
    if (use_crop && tr_outside(sm.xyz_f[3 * i], sm.xyz_f[3 * i + 2], lim)) {
      s1 = TR_CROPPED;
      if (live) sm.sigma_f[i] = s1;
    }
    s_key[wv][Nc + lane] = tr_key(t1);
  }
  __syncthreads();

  // ---- rank by counting: every lane reads the same key (an LDS broadcast) ----------------------------------------------------
  {
    const uint32_t k0 = tr_key(t0), k1 = tr_key(t1);
    int rank0 = 0, rank1 = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t kj = s_key[wv][j];
      rank0 += (kj < k0 || (kj == k0 && j < lane)) ? 1 : 0;
      rank1 += (kj < k1 || (kj == k1 && j < Nc + lane)) ? 1 : 0;
    }
    if (lane < Nc) { s_t[wv][rank0] = t0; s_s[wv][rank0] = s0; s_i[wv][rank0] = lane; }
    if (lane < Ni) { s_t[wv][rank1] = t1; s_s[wv][rank1] = s1; s_i[wv][rank1] = Nc + lane; }
  }
  __syncthreads();

  // ---- march: intervals p = lane (A) and 64 + lane (B) ------------------------------------------------------------------------
  float aA = 0.0f, mA = 0.0f, aB = 0.0f, mB = 0.0f;
  double fA = 1.0, fB = 1.0;
  if (lane < nm) {
    aA = tr_alpha(s_t[wv][lane], s_s[wv][lane], s_t[wv][lane + 1], s_s[wv][lane + 1]);
    mA = (s_t[wv][lane] + s_t[wv][lane + 1]) / 2.0f;
    fA = (double)((1.0f - aA) + 1e-10f);
  }
  const int pB = 64 + lane;
  if (pB < nm) {
    aB = tr_alpha(s_t[wv][pB], s_s[wv][pB], s_t[wv][pB + 1], s_s[wv][pB + 1]);
    mB = (s_t[wv][pB] + s_t[wv][pB + 1]) / 2.0f;
    fB = (double)((1.0f - aB) + 1e-10f);
  }
  const double inclA = tr_scan_mul(fA, lane);
  double throughA = __shfl_up(inclA, 1);
  if (lane == 0) throughA = 1.0;
  const float wA = lane < nm ? aA * (float)throughA : 0.0f;
  float wB = 0.0f;
  if (nm > 64) {                                    // wave-uniform
    const double inclB = tr_scan_mul(fB, lane);
    double throughB = __shfl_up(inclB, 1);
    if (lane == 0) throughB = 1.0;
    throughB = __shfl(inclA, 63) * throughB;
    if (pB < nm) wB = aB * (float)throughB;
  }
  s_w[wv][lane] = wA;
  s_w[wv][pB] = wB;
  const float wt = (float)tr_sum((double)wA + (double)wB);
  const float dt = (float)tr_sum((double)(wA * mA) + (double)(wB * mB));
  if (live && lane == 0) {
    float d = dt / wt;
    if (d != d) d = INFINITY;                       // nan_to_num(., inf); the clamp follows in tr_clamp_kernel
    weights[r] = wt;
    depth[r] = d;
    range[2 * r] = s_t[wv][0];
    range[2 * r + 1] = s_t[wv][nm];
  }
  __syncthreads();

  // ---- features: channel c on lanes c and 32 + c, each half one half of the intervals, front to back --------------------------
  {
    const int c = lane & 31, half = lane >> 5;
    const int split = (nm + 1) >> 1;
    const int p0 = half ? split : 0, p1 = half ? nm : split;
    auto row = [&](int p) -> float {
      const int i = s_i[wv][p];
      return i < Nc ? sm.rgb_c[(r * Nc + i) * TR_RGB + c] : sm.rgb_f[(r * Ni + (i - Nc)) * TR_RGB + c];
    };
    double acc = 0.0;
    float prev = row(p0);
#pragma unroll 4
    for (int p = p0; p < p1; ++p) {
      const float next = row(p + 1);
      acc += (double)(s_w[wv][p] * ((prev + next) / 2.0f));
      prev = next;
    }
    const double other = __shfl_xor(acc, 32);
    float f = (float)(half ? other + acc : acc + other);      // front half + back half in both lanes
    if (white_back) f = (f + 1.0f) - wt;
    if (live && half == 0) features[r * TR_RGB + c] = f;
  }
}

// the depth range of the call and the clamp: one workgroup (M rays -> 2 M floats read, M clamped)
__global__ __launch_bounds__(1024) void tr_clamp_kernel(int M, const float* __restrict__ range, float* __restrict__ depth) {
  __shared__ float s_lo[16], s_hi[16];
  const int tid = threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < M; i += 1024) { lo = fminf(lo, range[2 * i]); hi = fmaxf(hi, range[2 * i + 1]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
  if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); }
  for (int i = tid; i < M; i += 1024) depth[i] = fminf(fmaxf(depth[i], lo), hi);
}

}  // namespace

extern "C" int ggd_teacher_render(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                                  int32_t axes, float box_warp, const float* w1, const float* b1, const float* w2,
                                  const float* b2, int32_t rgb_act, const float* origins, const float* dirs, int32_t M,
                                  double ray_start, double ray_end, const float* coarse_table, int32_t Nc, int32_t Ni,
                                  const float* u_coarse, const float* u_fine, int32_t use_crop, double crop_limit,
                                  int32_t white_back, float* features, float* depth, float* weights, float* samples) {
  if (!ctx) return GGD_E_INVALID;
  const char* who = "ggd_teacher_render";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (Nc < TR_MIN_COARSE || Nc > TR_MAX || Ni < 0 || Ni > TR_MAX)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_teacher_render: 4 <= depth_resolution <= 64 and 0 <= depth_resolution_importance <= 64");
  if (!(ray_start < ray_end) || !std::isfinite(ray_start) || !std::isfinite(ray_end))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_teacher_render: finite ray_start < ray_end expected");
  if (use_crop && !std::isfinite(crop_limit)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_teacher_render: bad crop limit");
  if (M < 0 || (int64_t)M * (Nc + Ni) >= ((int64_t)1 << 31))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_teacher_render: 0 <= rays, rays * samples < 2^31");
  // the field's own refusals (channels, axes, depth, activation), before anything is launched
  const ggd_plane_set ps = {.grids_cl = grids_cl, .C = C, .D = D, .H = H, .W = W, .axes = axes, .box_warp = box_warp};
  const ggd_field_weights fw = {.w1 = w1, .b1 = b1, .w2 = w2, .b2 = b2, .act = rgb_act};
  int rc = ggd_check_field(ctx, who, ps, fw);
  if (rc != GGD_OK) return rc;
  if (M == 0) return GGD_OK;
  if (!grids_cl || !w1 || !b1 || !w2 || !b2 || H <= 0 || W <= 0 || box_warp == 0.0f || !origins || !dirs || !coarse_table ||
      !u_coarse || (Ni > 0 && !u_fine) || !features || !depth || !weights || (reinterpret_cast<uintptr_t>(samples) & 15))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_teacher_render: bad argument");

  const size_t nc = (size_t)M * Nc, nf = (size_t)M * Ni;
  const size_t block = (nc + nf) * (TR_RGB + 1 + 1 + 3);               // floats of the sample block
  rc = ggd_reserve_scratch(ctx, ((samples ? 0 : block) + 2 * (size_t)M) * sizeof(float), s);
  if (rc != GGD_OK) return rc;
  float* base = samples ? samples : static_cast<float*>(ctx->scratch);
  float* range = samples ? static_cast<float*>(ctx->scratch) : base + block;
  TrSamples sm;                                                          // the order of the block (include/ggd_raster.h)
  sm.rgb_c = base;               sm.rgb_f = sm.rgb_c + nc * TR_RGB;
  sm.sigma_c = sm.rgb_f + nf * TR_RGB;  sm.sigma_f = sm.sigma_c + nc;
  sm.depth_c = sm.sigma_f + nf;  sm.depth_f = sm.depth_c + nc;
  sm.xyz_c = sm.depth_f + nf;    sm.xyz_f = sm.xyz_c + 3 * nc;

  TrTable tab;
  for (int k = 0; k < TR_MAX; ++k) tab.t[k] = k < Nc ? coarse_table[k] : 0.0f;
  const float delta = (float)((ray_end - ray_start) / (double)(Nc - 1));
  const float lim = use_crop ? (float)crop_limit : 0.0f;
  const dim3 rays((unsigned)((M + TR_RAYS - 1) / TR_RAYS)), wg(64 * TR_RAYS);

  hipLaunchKernelGGL(tr_coarse_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, tab, delta, Nc, (int64_t)nc, origins, dirs,
                     u_coarse, sm.depth_c, sm.xyz_c);
  GGD_HIP(hipGetLastError());
  rc = ggd_launch_density_points(ctx, s, who, ps, fw, sm.xyz_c, (int64_t)nc, sm.sigma_c, sm.rgb_c);
  if (rc != GGD_OK) return rc;
  if (Ni > 0) {
    hipLaunchKernelGGL(tr_importance_kernel, rays, wg, 0, s, M, Nc, Ni, use_crop, lim, origins, dirs, u_fine, sm);
    GGD_HIP(hipGetLastError());
    rc = ggd_launch_density_points(ctx, s, who, ps, fw, sm.xyz_f, (int64_t)nf, sm.sigma_f, sm.rgb_f);
    if (rc != GGD_OK) return rc;
  }
  hipLaunchKernelGGL(tr_composite_kernel, rays, wg, 0, s, M, Nc, Ni, use_crop, lim, white_back, sm, features, depth, weights, range);
  GGD_HIP(hipGetLastError());
  hipLaunchKernelGGL(tr_clamp_kernel, dim3(1), dim3(1024), 0, s, M, range, depth);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
