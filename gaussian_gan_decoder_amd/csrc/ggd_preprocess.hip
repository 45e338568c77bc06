// ggd_preprocess.hip -- stage a4 (per-Gaussian forward) and a12 (mark_visible) for gfx950.
//
// Replaces the per-Gaussian half of `_C.rasterize_gaussians` that the reference reaches through
// gaussian_splatting/gaussian_renderer/__init__.py:167-175 (source not in the reference tree; algorithm restated
// in SURVEY.md section 9.2).  One lane per Gaussian, 256-lane workgroups that each walk several 256-Gaussian tiles (a persistent
// grid); every input array is read exactly once
// with per-lane vector loads over contiguous addresses (a wave covers 64 consecutive Gaussians = one contiguous
// 768 B / 1 KiB span per array), and the outputs the blend needs are packed into ONE 48-byte record per Gaussian
// (ggd_splat) so that the per-tile gather later touches a single 64 B-aligned-ish record instead of four arrays.
// HBM-bound: 56 B in (degree 0) + 56 B out per visible Gaussian, 56 B in + 8 B out per culled one.
#include "ggd_math.h"
#include "ggd_lanes.h"

namespace {
using namespace ggdm;

// SHVEC (more than the band-0 coefficient per channel, rows a multiple of 16 bytes: M = 4, 8, 12, 16): a visible Gaussian's
// 3 M coefficients are fetched as 3 M / 4 dwordx4 loads into registers instead of 3 M lone words -- each such load
// instruction touches 64 different rows whatever its width (1 M Gaussians, M = 16: preprocess 76 -> see DESIGN.md).
// FOLD (ggd_fold, single-call forward on the tile-binning path): the workgroup also (a) clears its share of the OTHER
// control block for the next frame, (b) adds the four digit counts of its kept depth keys to replica blockIdx % REPS of the
// depth sort's histograms (LDS histogram over all its tiles first, one flush; bins that stayed empty cost nothing), (c) stores
// {sum of tiles_touched, kept keys} of each tile's 256 points for the offsets scan -- the sort's histogram launch and the scan's
// first step disappear.
// AA (ggd_params.antialiasing): the opacity-compensated 2D filter.  The record's opacity -- and with it thr, ex, ey -- is
// o_eff = o h, h = sqrt(max(2.5e-5, det0 / det1)), det0 / det1 the determinants of the EWA 2D covariance before / after the
// 0.3 px^2 dilation (Mip-Splatting).  The conic, radius, rect, tiles_touched and depth key come from the dilated covariance
// either way.
// Workgroups per compute unit of the persistent grid: 6 and 7 measured alike (the kernel holds 7 waves per SIMD), 4 and 2 slower
// (DESIGN.md section 6q).
constexpr int GGD_PREPROCESS_WGS_PER_CU = 6;

// What the kernel reads of every Gaussian whatever becomes of it: position, scale, rotation, colour (or SH band 0), opacity.
typedef float f3v __attribute__((ext_vector_type(3)));
typedef float f4v __attribute__((ext_vector_type(4)));
struct pre_inputs { f3v p, s, c; f4v q; float o; };

// The kernel's one argument.  The kernel walks many tiles, and forty arguments held in registers around that loop -- with
// everything the compiler derives from them once -- cost it 16 scalar registers spilled and two waves per SIMD.  So each tile
// reads what it needs from the kernel-argument segment again, as a one-tile kernel does (tile_args()), in front of the wait
// for its inputs.
struct pre_args {
  int P, M, deg, W, H;
  float tanfovx, tanfovy, fx, fy, mod;
  int prefiltered, raw;
  const float *view, *proj, *campos, *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
  ggd_splat* splat;
  uint32_t* tiles_touched;
  uint8_t* clamped;
  int32_t* radii;
  uint32_t* depth_keys;
  uint2* rect;
  uint32_t* trap_flag;
  uint32_t* zero_ptr;
  int zero_words;
  ggd_fold fold;
};
typedef const __attribute__((address_space(4))) pre_args* pre_args_ptr;

// The argument segment (pre_args is the kernel's first and only explicit argument: offset 0) as a pointer the compiler cannot
// trace from one tile to the next: no load through it is hoisted out of the tile loop.
__device__ __forceinline__ pre_args_ptr tile_args() {
  pre_args_ptr a = (pre_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}
// A pointer read through tile_args() is a generic one to the compiler; every one of them points to device memory.
template <typename T>
__device__ __forceinline__ T* as_global(T* p) {
  return (T*)(__attribute__((address_space(1))) T*)p;
}

// Requests a tile's inputs and does NOT wait for them: `in` is not to be read, copied or passed on before landed(in) has
// returned.  Inline asm, because the compiler sinks plain loads behind the culling tests (their only uses).  An array this call
// does not have is replaced by the 64-byte view matrix, so that no load sits behind a branch; the lanes behind P of the last tile
// read Gaussian P - 1 and use nothing of it.
__device__ __forceinline__ void request_inputs(pre_inputs& in, int tile) {
  const pre_args_ptr a = tile_args();
  const int i = min(tile * 256 + (int)threadIdx.x, a->P - 1);
  const float* view = as_global(a->view);
  const float* colors_precomp = as_global(a->colors_precomp);
  const float* shs = as_global(a->shs);
  const bool cov = a->cov3D_precomp != nullptr;
  const float* pp = as_global(a->means3D) + 3 * (size_t)i;
  const float* sp = cov ? view : as_global(a->scales) + 3 * (size_t)i;
  const float* qp = cov ? view : as_global(a->rotations) + 4 * (size_t)i;
  const float* cp = colors_precomp ? colors_precomp + 3 * (size_t)i : (shs ? shs + (size_t)i * a->M * 3 : view);   // colour, or SH band 0
  const float* op = as_global(a->opacities) + i;
  asm volatile("global_load_dwordx3 %0, %5, off\n\t"
               "global_load_dwordx3 %1, %6, off\n\t"
               "global_load_dwordx4 %2, %7, off\n\t"
               "global_load_dwordx3 %3, %8, off\n\t"
               "global_load_dword %4, %9, off"
               : "=&v"(in.p), "=&v"(in.s), "=&v"(in.q), "=&v"(in.c), "=&v"(in.o)
               : "v"(pp), "v"(sp), "v"(qp), "v"(cp), "v"(op)
               : "memory");
}
// The hardware completes loads in order, but stores issued earlier (the control-block clear, the tile before) share the counter:
// one wait for everything.  Then every register of `in` passes through an empty statement: nothing that reads one can be
// scheduled ahead of the wait, and a copy the compiler makes for the statement's sake sits behind the wait too.
__device__ __forceinline__ void landed(pre_inputs& in) {
  asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
  asm volatile("" : "+v"(in.p), "+v"(in.s), "+v"(in.q), "+v"(in.c), "+v"(in.o) : : "memory");
}

template <bool SHVEC, bool FOLD, bool AA = false>
__global__ __launch_bounds__(256) void preprocess_kernel(pre_args args) {
  __shared__ uint32_t s_hist[FOLD ? GGD_FOLD_REP_STRIDE : 1];
  // two buffers of 16 (tile parity), per wave: sum of tiles, kept keys, ~min key, max key; [32]: keys outside the window
  __shared__ uint32_t s_red[FOLD ? 33 : 1];
  __shared__ int s_rowdiff[FOLD ? 65 : 1];
  __shared__ int s_rowwdiff[FOLD ? 65 : 1];   // the same difference array weighted by the rect's width: instances per tile row
  // Persistent grid: the workgroup takes the 256-Gaussian tiles blockIdx.x, blockIdx.x + gridDim.x, ...  What is keyed by the
  // tile (the per-Gaussian stores, fold.wg_info[tile]) is written per tile, what is a sum (the histograms, the row arrays, the
  // outside count) stays in LDS until the workgroup ends: one flush per workgroup, not per tile.
  const Mat16 V = load_mat(args.view);   // (ahead of every store: scalar loads)
  const Mat16 PV = load_mat(args.proj);
  const int tiles = (args.P + 255) >> 8;
  int tile = blockIdx.x;
  int parity = 0;
  pre_inputs in;
  request_inputs(in, tile);   // in flight under the clears and the barrier below
  if constexpr (FOLD) {
    for (uint32_t z = blockIdx.x * 256 + threadIdx.x; z < args.fold.clear_words; z += gridDim.x * 256) args.fold.clear[z] = 0u;
    for (int b = threadIdx.x; b < GGD_FOLD_REP_STRIDE; b += 256) s_hist[b] = 0u;
    if (threadIdx.x < 65) { s_rowdiff[threadIdx.x] = 0; s_rowwdiff[threadIdx.x] = 0; }
    if (threadIdx.x == 0) s_red[32] = 0u;
    __syncthreads();
  } else {
    // first kernel of a frame: its first workgroups also clear the depth sort's control block (no memset launch there)
    const int zb = min(8, (int)gridDim.x);
    if ((int)blockIdx.x < zb)
      for (int z = blockIdx.x * 256 + threadIdx.x; z < args.zero_words; z += zb * 256) args.zero_ptr[z] = 0u;
  }
  auto do_tile = [&](pre_inputs& cur, const int tile, const int parity) __attribute__((always_inline)) {
  const pre_args_ptr a = tile_args();
  const int P = a->P, M = a->M, deg = a->deg, W = a->W, H = a->H, prefiltered = a->prefiltered, raw = a->raw;
  const float tanfovx = a->tanfovx, tanfovy = a->tanfovy, fx = a->fx, fy = a->fy, mod = a->mod;
  const float* campos_p = as_global(a->campos);
  const float* shs = as_global(a->shs);
  const float* colors_precomp = as_global(a->colors_precomp);
  const float* cov3D_precomp = as_global(a->cov3D_precomp);
  ggd_splat* splat = as_global(a->splat);
  uint32_t* tiles_touched = as_global(a->tiles_touched);
  uint8_t* clamped = as_global(a->clamped);
  int32_t* radii = as_global(a->radii);
  uint32_t* depth_keys = as_global(a->depth_keys);
  uint2* rect = as_global(a->rect);
  uint32_t* trap_flag = as_global(a->trap_flag);
  // The arguments arrive while the tile's inputs are still on their way: read behind the wait, "at the point of use", they
  // are three dependent scalar round trips on the tile's critical path (+ 1.4 us on a 391-workgroup launch).
  asm volatile("" : : "s"(P), "s"(M), "s"(deg), "s"(W), "s"(H), "s"(prefiltered), "s"(raw), "s"(tanfovx), "s"(tanfovy), "s"(fx),
               "s"(fy), "s"(mod), "s"(shs), "s"(colors_precomp), "s"(cov3D_precomp));
  asm volatile("" : : "s"(splat), "s"(tiles_touched), "s"(clamped), "s"(radii), "s"(depth_keys), "s"(rect), "s"(trap_flag));
  landed(cur);
  const int i = tile * 256 + threadIdx.x;
  const bool in_range = i < P;
  // Every per-Gaussian input was requested in one go, whatever the culling tests below decide: behind the tests
  // (position -> depth test -> scale / rotation -> rect test -> colour -> opacity) a wave paid four dependent trips to memory
  // and lived 10 us, 60 % of it waiting.  The price is 16 B of colour + opacity for a Gaussian whose rect turns out empty.
  int irad = 0;
  uint32_t ntiles = 0, rect_rows = 0, rect_cols = 0;   // rect_rows = miny | maxy << 16, rect_cols = minx | maxx << 16 of a visible Gaussian
  bool visible = false;
  float depth = 0.0f;
  if (in_range) {
  const float opac_in = cur.o;
  const float p[3] = {cur.p.x, cur.p.y, cur.p.z};
  float s3[3] = {cur.s.x, cur.s.y, cur.s.z};
  float4 q = make_float4(cur.q.x, cur.q.y, cur.q.z, cur.q.w);
  const float rgb_in[3] = {cur.c.x, cur.c.y, cur.c.z};
  float t[3];
  t[0] = V.m[0] * p[0] + V.m[4] * p[1] + V.m[8] * p[2] + V.m[12];
  t[1] = V.m[1] * p[0] + V.m[5] * p[1] + V.m[9] * p[2] + V.m[13];
  t[2] = V.m[2] * p[0] + V.m[6] * p[1] + V.m[10] * p[2] + V.m[14];
  depth = t[2];

  ggd_splat out;
  uint32_t clamp_bits = 0;
  uint2 rect_out = make_uint2(0u, 0u);

  if (t[2] > 0.2f) {
    float h[4];
    h[0] = PV.m[0] * p[0] + PV.m[4] * p[1] + PV.m[8] * p[2] + PV.m[12];
    h[1] = PV.m[1] * p[0] + PV.m[5] * p[1] + PV.m[9] * p[2] + PV.m[13];
    h[3] = PV.m[3] * p[0] + PV.m[7] * p[1] + PV.m[11] * p[2] + PV.m[15];
    const float pw = 1.0f / (h[3] + 0.0000001f);
    const float ndcx = h[0] * pw, ndcy = h[1] * pw;

    float c6[6];
    if (cov3D_precomp) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * (size_t)i + k];
    } else {
      if (raw) {
        float nrm;
        s3[0] = expf(s3[0]); s3[1] = expf(s3[1]); s3[2] = expf(s3[2]);
        q = act_normalize(q, nrm);
      }
      cov3d_from_scale_rot(s3, mod, q, c6);
    }
    float abc[3], Tm[2][3], tcl[3];
    bool clx, cly;
    ewa_cov2d(t, fx, fy, tanfovx, tanfovy, c6, V, abc, Tm, tcl, clx, cly);
    const float a = abc[0] + 0.3f, b = abc[1], c = abc[2] + 0.3f;
    const float det = a * c - b * b;
    if (det != 0.0f) {
      const float det_inv = 1.0f / det;
      const float mid = 0.5f * (a + c);
      const float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
      const float lambda1 = mid + disc, lambda2 = mid - disc;
      const float my_radius = ceilf(3.0f * sqrtf(fmaxf(lambda1, lambda2)));
      const float px = ((ndcx + 1.0f) * (float)W - 1.0f) * 0.5f;
      const float py = ((ndcy + 1.0f) * (float)H - 1.0f) * 0.5f;
      const int r_i = (int)my_radius;
      int minx, miny, maxx, maxy;
      const int gx = (W + 15) / 16, gy = (H + 15) / 16;
      const int area = ggd_tile_rect(px, py, r_i, gx, gy, minx, miny, maxx, maxy);
      if (area != 0) {
        visible = true;
        irad = r_i;
        ntiles = (uint32_t)area;
        float rgb[3];
        if (colors_precomp) {
          rgb[0] = rgb_in[0]; rgb[1] = rgb_in[1]; rgb[2] = rgb_in[2];
        } else if (deg == 0) {   // band 0 only (what the decoder's renderer passes): the coefficients arrived with the rest
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float res = SH_C0 * rgb_in[c] + 0.5f;
            if (res < 0.0f) clamp_bits |= (1u << c);
            rgb[c] = fmaxf(res, 0.0f);
          }
        } else {
          const float campos[3] = {campos_p[0], campos_p[1], campos_p[2]};
          if constexpr (SHVEC) {
            float shr[48];
            const float4* src = reinterpret_cast<const float4*>(shs + (size_t)i * M * 3);
            const int nq = (3 * M) >> 2;
#pragma unroll
            for (int qd = 0; qd < 12; ++qd) {
              float4 v = make_float4(0, 0, 0, 0);
              if (qd < nq) v = src[qd];
              shr[4 * qd] = v.x; shr[4 * qd + 1] = v.y; shr[4 * qd + 2] = v.z; shr[4 * qd + 3] = v.w;
            }
            sh_to_rgb(deg, shr, p, campos, rgb, clamp_bits);
          } else {
            sh_to_rgb(deg, shs + (size_t)i * M * 3, p, campos, rgb, clamp_bits);
          }
        }
        rect_out = make_uint2((uint32_t)minx | ((uint32_t)maxx << 16), (uint32_t)miny | ((uint32_t)maxy << 16));
        const float conA = c * det_inv, conB = -b * det_inv, conC = a * det_inv;   // the published conic
        float opac = raw ? act_sigmoid(opac_in) : opac_in;
        if constexpr (AA) {   // o_eff = o h; correctly rounded division and square root (build flags), like the
          const float det0 = abc[0] * abc[2] - abc[1] * abc[1];   // bit-exact fields around it
          opac = opac * sqrtf(fmaxf(2.5e-5f, det0 / det));
        }
        out.x = px; out.y = py;
        out.hA = -0.5f * conA; out.nB = -conB; out.hC = -0.5f * conC;   // exact rescalings (see ggd_raster.h)
        out.opacity = opac;
        out.r = rgb[0]; out.g = rgb[1]; out.b = rgb[2];
        // Blend-side culling data, once per Gaussian (the blend kernels used to derive it once per (tile, Gaussian)):
        // alpha = opacity * exp(power) >= 1/255  <=>  power >= L = ln(1 / (255 opacity)); thr sits a safety margin below L so
        // that the decision is exact w.r.t. the float alpha test that follows.  {power >= thr} is the ellipse
        // d^T Q d <= tau2 = -2 thr, Q = [[A, B], [B, C]]; its axis-aligned half extents are sqrt(tau2 C / det),
        // sqrt(tau2 A / det), inflated by 1.001 + 4e-6 trace^2 / det (the fp32 rounding of the in-loop power evaluation
        // grows with the anisotropy of Q) + 0.01 px.  Indefinite / NaN conics get +inf (never culled by the box);
        // thr > 0 (opacity < 1/255) can never be reached by power <= 0: the box is empty (extents -inf).
        // (hardware log / reciprocal / square root here, not the correctly rounded forms the bit-exact outputs above need: this
        // block only has to be conservative, its 1-2 ulp are three orders below the margins -- 28.2 -> 25.9 us at 1 M points)
        const float L = -__logf(255.0f * opac);
        float thr = L - (2e-5f + 1e-6f * fabsf(L));
        const float cdet = conA * conC - conB * conB;
        const float tau2 = -2.0f * thr;
        float ex = __builtin_huge_valf(), ey = __builtin_huge_valf();
        if (cdet > 0.0f) {
          const float rc = __builtin_amdgcn_rcpf(cdet);
          const float sdet = tau2 * rc;
          const float tr = conA + conC;
          const float infl = 1.001f + 4e-6f * (tr * tr) * rc;
          ex = __builtin_amdgcn_sqrtf(fmaxf(sdet * conC, 0.0f)) * infl + 0.01f;
          ey = __builtin_amdgcn_sqrtf(fmaxf(sdet * conA, 0.0f)) * infl + 0.01f;
        }
        if (tau2 < 0.0f) { ex = -__builtin_huge_valf(); ey = -__builtin_huge_valf(); }
        // opacity <= 0 (or NaN): L is +inf / NaN and thr = inf - inf = NaN.  alpha = opacity * G <= 0 < 1/255 for every
        // pixel, so the record can never contribute: say so explicitly (threshold +inf, empty box) instead of relying
        // on how the three blend kernels' comparisons treat a NaN threshold
        if (!(opac > 0.0f) || !(L < __builtin_huge_valf())) {
          thr = __builtin_huge_valf(); ex = -__builtin_huge_valf(); ey = -__builtin_huge_valf();
        }
        out.thr = thr; out.ex = ex; out.ey = ey;
      }
    }
  } else if (prefiltered) {
    atomicOr(trap_flag, 1u);  // upstream traps here; we report GGD_E_PREFILTER instead
  }

  radii[i] = irad;
  tiles_touched[i] = ntiles;
  depth_keys[i] = visible ? __float_as_uint(t[2]) : 0xFFFFFFFFu;
  rect[i] = rect_out;
  rect_rows = rect_out.y; rect_cols = rect_out.x;
  if (clamped) clamped[i] = (uint8_t)clamp_bits;
  if (visible) {
    float4* dst = reinterpret_cast<float4*>(splat + i);
    const float4* src = reinterpret_cast<const float4*>(&out);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  }
  }  // in_range
  if constexpr (FOLD) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t key = __float_as_uint(depth);
    const uint64_t act = __ballot(visible);
    if (act != 0ull) {
      // (as sort_global_hist_kernel: the two high bytes -- sign / exponent / leading mantissa bits of a depth -- are usually
      // shared by the whole wave: one lane adds the count instead of 64 conflicting LDS atomics)
      const int leader = __builtin_ctzll(act);
      if (a->fold.msd) {   // two-launch sort: the bucket inside the key window (never shared by a wave) and the top byte (almost always)
        if (visible) {
          const uint32_t bkt = (key - a->fold.msd_lo) >> a->fold.msd_shift;     // (a key below the window wraps to a huge value)
          atomicAdd(&s_hist[min(bkt, (uint32_t)(GGD_MSD_BINS - 1))], 1u);
          if (bkt > (uint32_t)(GGD_MSD_BINS - 1)) atomicAdd(&s_red[32], 1u);   // outside: the frame will be rendered again
        }
        const uint32_t d = key >> 24;
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
        if (__ballot(visible && d != d0) == 0ull) {
          if (lane == leader) atomicAdd(&s_hist[GGD_MSD_BINS + d0], (uint32_t)__popcll(act));
        } else if (visible) {
          atomicAdd(&s_hist[GGD_MSD_BINS + d], 1u);
        }
      } else
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const uint32_t d = (key >> (8 * pass)) & 0xffu;
        if (pass < 2) {
          if (visible) atomicAdd(&s_hist[pass * 256 + d], 1u);
          continue;
        }
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
        if (__ballot(visible && d != d0) == 0ull) {
          if (lane == leader) atomicAdd(&s_hist[pass * 256 + d0], (uint32_t)__popcll(act));
        } else if (visible) {
          atomicAdd(&s_hist[pass * 256 + d], 1u);
        }
      }
    }
    // (d) grids of <= 64 tile rows: entries per row for the row binning's first level -- difference array over the rows the
    //     Gaussian's rect covers, prefix over the lanes after the barrier; and the INSTANCES per row (each entry weighted by the
    //     rect's width) for its second level.  visible <=> rect area > 0 <=> level 1 emits the Gaussian's entries: the tile
    //     starts behind a Gaussian counted here and not binned there would all shift.
    if (a->fold.rows && visible) {
      const int w = (int)(rect_cols >> 16) - (int)(rect_cols & 0xffffu);
      atomicAdd(&s_rowdiff[rect_rows & 0xffffu], 1);
      atomicAdd(&s_rowdiff[rect_rows >> 16], -1);
      atomicAdd(&s_rowwdiff[rect_rows & 0xffffu], w);
      atomicAdd(&s_rowwdiff[rect_rows >> 16], -w);
    }
    uint32_t tsum = ntiles;
    // kept-key range of the frame (for the NEXT frames' two-launch-sort window): ~min and max, so that both reduce -- and
    // accumulate in the zeroed control block -- as maxima
    uint32_t nmin = visible ? ~key : 0u, kmax = visible ? key : 0u;
    tsum = wave_sum_lane63(tsum); nmin = wave_max_lane63(nmin); kmax = wave_max_lane63(kmax);   // (lane 63 writes them)
    // (the tile after this one writes the other buffer, and nobody writes this one again before thread 0 has passed the next
    // tile's barrier: one barrier per tile)
    uint32_t* red = s_red + 16 * parity;
    if (lane == 63) { red[wv] = tsum; red[4 + wv] = (uint32_t)__popcll(act); red[8 + wv] = nmin; red[12 + wv] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0)
      as_global(a->fold.wg_info)[tile] = make_uint4(red[0] + red[1] + red[2] + red[3], red[4] + red[5] + red[6] + red[7],
                                      max(max(red[8], red[9]), max(red[10], red[11])),
                                      max(max(red[12], red[13]), max(red[14], red[15])));
  }
  };  // do_tile
  for (;;) {
    do_tile(in, tile, parity);
    tile += gridDim.x;
    if (tile >= tiles) break;
    parity ^= 1;
    request_inputs(in, tile);
  }
  if constexpr (FOLD) {   // (behind the last tile's barrier: every LDS sum is complete)
    const int lane = threadIdx.x & 63;
    const pre_args_ptr a = tile_args();
    uint32_t* ctl = as_global(a->fold.ctl);
    uint32_t* hist = ctl + (blockIdx.x % GGD_FOLD_REPS) * GGD_FOLD_REP_STRIDE;
    const int used = a->fold.msd ? GGD_FOLD_REP_STRIDE : 4 * 256;
    for (int b = threadIdx.x; b < used; b += 256) {
      const uint32_t c = s_hist[b];
      if (c) atomicAdd(&hist[b], c);
    }
    if (a->fold.rows && threadIdx.x < 64) {
      const int c = wave_inclusive_scan(s_rowdiff[lane]), cw = wave_inclusive_scan(s_rowwdiff[lane]);
      if (c) {   // (a row without entries has no instances)
        atomicAdd(&ctl[GGD_FOLD_ROWTOT + (blockIdx.x % GGD_FOLD_REPS) * 64 + lane], (uint32_t)c);
        atomicAdd(&as_global(a->fold.rowinst)[(blockIdx.x % GGD_FOLD_REPS) * 64 + lane], (uint32_t)cw);
      }
    }
    if (threadIdx.x == 0 && s_red[32]) atomicAdd(&ctl[GGD_FOLD_OUTSIDE], s_red[32]);
  }
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

int ggd_launch_preprocess(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_inputs& in, ggd_splat* splat,
                          uint32_t* tiles_touched, uint8_t* clamped, int32_t* radii, uint32_t* depth_keys, uint2* rect, uint32_t* trap_flag, uint32_t* zero_ptr, int zero_words,
                          const ggd_fold* fold) {
  if (prm.P == 0) return GGD_OK;
  // persistent grid: GGD_PREPROCESS_WGS_PER_CU workgroups per compute unit stride over the 256-Gaussian
  // tiles; GGD_OPT_PREPROCESS_WGS = n > 0 asks for exactly min(n, tiles) workgroups
  const int tiles = (prm.P + 255) / 256;
  const int want = ctx->opt[GGD_OPT_PREPROCESS_WGS] > 0 ? ctx->opt[GGD_OPT_PREPROCESS_WGS] : GGD_PREPROCESS_WGS_PER_CU * ctx->cus;
  const int grid = min(tiles, max(want, 1));
  const bool shvec = !in.colors_precomp && prm.M > 1 && prm.M <= 16 && ((3 * prm.M) & 3) == 0;
  const ggd_fold f = fold ? *fold : ggd_fold{};
  // focal lengths: wave-uniform correctly rounded divisions, done once here (same fp32 expression, same result)
  const float fx = (float)prm.width / (2.0f * prm.tanfovx), fy = (float)prm.height / (2.0f * prm.tanfovy);
  pre_args a{};
  a.P = prm.P; a.M = prm.M; a.deg = prm.sh_degree; a.W = prm.width; a.H = prm.height;
  a.tanfovx = prm.tanfovx; a.tanfovy = prm.tanfovy; a.fx = fx; a.fy = fy; a.mod = prm.scale_modifier;
  a.prefiltered = prm.prefiltered; a.raw = prm.raw_attributes;
  a.view = prm.viewmatrix; a.proj = prm.projmatrix; a.campos = prm.campos;
  a.means3D = in.means3D; a.shs = in.shs; a.colors_precomp = in.colors_precomp; a.opacities = in.opacities; a.scales = in.scales;
  a.rotations = in.rotations; a.cov3D_precomp = in.cov3D_precomp;
  a.splat = splat; a.tiles_touched = tiles_touched; a.clamped = clamped; a.radii = radii; a.depth_keys = depth_keys; a.rect = rect;
  a.trap_flag = trap_flag; a.zero_ptr = zero_ptr; a.zero_words = zero_ptr ? zero_words : 0;
  a.fold = f;
  ggd_dispatch<2>(shvec, [&](auto sv) {
    ggd_dispatch<2>(fold != nullptr, [&](auto fo) {
      ggd_dispatch<2>(prm.antialiasing != 0, [&](auto aa) {
        hipLaunchKernelGGL((preprocess_kernel<decltype(sv)::value != 0, decltype(fo)::value != 0, decltype(aa)::value != 0>),
                           dim3(grid), dim3(256), 0, s, a);
      });
    });
  });
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
