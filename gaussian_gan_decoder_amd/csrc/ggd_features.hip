// ggd_features.hip -- N-channel feature maps blended over the contributors of a finished colour render (ggd_forward_features /
// ggd_backward_features).
//
//   F_c = sum_i alpha_i T_i f_{i,c} + T_final b_c        c = 0 .. C - 1,  1 <= C <= 32
//
// The weight w_i = alpha_i T_i of a (pixel, contributor) pair is the colour pass's: both kernels walk the tile's sorted list as the
// colour blend does, bounded per pixel by the stored n_contrib, and recompute alpha with the colour kernels' own expressions
// (ggd_blend_math.h: blend_power, blend_exp<MODE>, blend_exp_backward<MODE>; pair_forward of ggd_quarter_walk.h and the backward
// kernel below: the same skip tests in the same order).  With -ffp-contract=off the same expression gives the same bits, so the set of contributors of a pixel is the colour
// pass's, pair by pair; inside the n_contrib bound no pixel meets the colour pass's T < 1e-4 stop again (the stop lies behind its
// last contributor).
//
// Shape of both kernels: the quarter walk of ggd_quarter_walk.h -- one single-wave workgroup per 8x8 quarter of a 16x16 tile, one
// pixel per lane, GGD_FEATURES_ROUND = 64 list entries per round, pre-culled and staged compacted by the gathering lanes.  What is
// this file's: all 64 lanes copy the staged records' feature rows f[id_j][0 .. C) into LDS once ([64][CG] floats, CG = C rounded up
// to 4 / 8 / 16 / 32; the padding channels are filled with zeros in LDS, never read from `features` and never written anywhere),
// and the C-wide parts, three small dense products per round, done as plain fp32 VALU loops over channels with the record side
// broadcast from LDS:
//   forward    F[pix, c]  += W[pix, rec] f[rec, c]                  (pixel per lane, F in CG registers)
//   backward   d[pix, rec] = sum_c G[pix, c] f[rec, c]              (pixel per lane, G = dL/dF of the pixel in CG registers)
//   backward   dL/df[rec, c] = sum_pix W[pix, rec] G[pix, c]        (record per lane: W parked per round in LDS, G staged once)
// After the second product the C-channel form of dL/dalpha collapses to the colour backward's scalar recurrence: with
// S = sum_c G_c acc_c (acc = the features composited behind the record) dL/dalpha's colour part is d - S, and S <- S + alpha (d - S).
// The per-record geometry sums (conic, opacity, mean) are formed by the record's lane from the parked q = G dL/dalpha and the
// pixel offsets it recomputes, scaled by bwd_scale and added to the EXISTING accumulator records (GGD_ACC_CONIC / _OPACITY / _MEAN2D), which the per-Gaussian
// backward reads once for every map.
#include "ggd_common.h"

namespace {

#include "ggd_blend_math.h"
#include "ggd_quarter_walk.h"

// One round's records (stage_cull) and the survivors' feature rows into LDS.  The rows depend on the cull's outcome; they are
// requested eight per lane before the first is waited for, and the gather's next loads -- the records of the next round, the list
// entries of the one after -- right behind the last batch of rows, so that they are in flight while this round is blended.
// Returns the number of staged records (wave-uniform).
template <int CG>
__device__ __forceinline__ int stage_round(float4* s_rec, uint32_t* s_id, float* s_f, Gather& ga, int n, uint32_t pos0,
                                           uint32_t pos_after_next, int C, int cull, const QuarterGeom& g,
                                           const float* __restrict__ features) {
  const int lane = threadIdx.x;
  const int ns = stage_cull(s_rec, s_id, ga, g, n, pos0, cull, [](int) {});
  __syncthreads();
  for (int t0 = 0; t0 < ns * CG; t0 += 64 * 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u * 64 + lane, j = t / CG, c = t - j * CG;
      v[u] = (t < ns * CG && c < C) ? features[(size_t)s_id[min(j, ROUND - 1)] * C + c] : 0.0f;
    }
    if (t0 + 64 * 8 >= ns * CG) {        // behind the last batch of rows
      ga.load_rec();
      ga.load_id(pos_after_next);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u * 64 + lane;
      if (t < ns * CG) s_f[t] = v[u];
    }
  }
  if (ns == 0) {
    ga.load_rec();
    ga.load_id(pos_after_next);
  }
  __syncthreads();
  return ns;
}

// ---- forward -------------------------------------------------------------------------------------------------------------
template <int EXP_MODE, int CG>
__global__ __launch_bounds__(64) void features_forward_kernel(int W, int H, int gx, int T, int C, int cull,
                                                              const ggd_splat* __restrict__ splat,
                                                              const uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ ranges, uint32_t R,
                                                              const uint32_t* __restrict__ n_contrib,
                                                              const float* __restrict__ features,
                                                              const float* __restrict__ feature_bg,
                                                              float* __restrict__ out) {
  __shared__ float4 s_rec[ROUND * 2];
  __shared__ uint32_t s_id[ROUND];
  __shared__ float s_f[ROUND * CG];
  const QuarterGeom g((int)blockIdx.x, W, H, gx, T, ranges, R, n_contrib);
  float F[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) F[c] = 0.0f;

  Gather ga(splat, list, g);
  const float Tr = walk_front<EXP_MODE>(
      s_rec, g, cull, ga,
      [&](int n, uint32_t pos0, uint32_t pos_after_next) {
        return stage_round<CG>(s_rec, s_id, s_f, ga, n, pos0, pos_after_next, C, cull, g, features);
      },
      [&](int j, const PairForward& p) {
        const float* f = s_f + j * CG;
#pragma unroll
        for (int c = 0; c < CG; ++c) F[c] = __builtin_fmaf(f[c], p.w, F[c]);
      });
  if (!g.in) return;
  const size_t HW = (size_t)H * W;
#pragma unroll
  for (int c = 0; c < CG; ++c)
    if (c < C) out[(size_t)c * HW + g.pix] = F[c] + Tr * (feature_bg ? feature_bg[c] : 0.0f);
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// EXP_MODE: the colour backward's (0 .. 3).  Records are visited back to front from the quarter's deepest last contributor; a
// pixel that does not see a record gets alpha = G = 0, which makes every state update an exact no-op (the colour backward's
// select-free body).  A round's staged records are taken in chunks of FLUSH = 32, from the back: the pixel lanes park
// w = alpha T and q = G dL/dalpha of every (record, pixel) pair of the chunk some pixel sees; then lane (j, h) = (lane & 31,
// lane >> 5) owns record j of the chunk -- half h of the channels of its dL/dfeatures row over all 64 pixels, and half h of the
// pixels of its six geometry sums, combined over the two halves with one cross-half exchange.
template <int EXP_MODE, int CG>
__global__ __launch_bounds__(64) void features_backward_kernel(int W, int H, int gx, int T, int C, int cull,
                                                               const ggd_splat* __restrict__ splat,
                                                               const uint32_t* __restrict__ list,
                                                               const uint32_t* __restrict__ ranges, uint32_t R,
                                                               const float* __restrict__ final_T,
                                                               const uint32_t* __restrict__ n_contrib,
                                                               const float* __restrict__ features,
                                                               const float* __restrict__ feature_bg,
                                                               const float* __restrict__ dL_dF,
                                                               float* __restrict__ grad_acc,
                                                               float* __restrict__ dL_dfeatures) {
  constexpr int CH = CG / 2;             // channels of a record's row per flush lane
  __shared__ float4 s_rec[ROUND * 2];
  __shared__ uint32_t s_id[ROUND];
  __shared__ float s_f[ROUND * CG];
  __shared__ float s_g[64 * CG];         // dL/dF of the quarter's pixels, [pixel][channel]
  __shared__ float s_w[FLUSH * WPAD];    // alpha T        of (record of the chunk, pixel)
  __shared__ float s_q[FLUSH * WPAD];    // G dL/dalpha    of (record of the chunk, pixel)
  const int lane = threadIdx.x;
  const QuarterGeom g((int)blockIdx.x, W, H, gx, T, ranges, R, n_contrib);
  const uint32_t lastn = g.lastn, maxn = g.maxn;
  if (maxn == 0) return;
  const size_t HW = (size_t)H * W;
  const float pxf = (float)g.px, pyf = (float)g.py;
  const float tf = g.in ? final_T[g.pix] : 0.0f;
  float gp[CG], bgdot = 0.0f;
#pragma unroll
  for (int c = 0; c < CG; ++c) {
    gp[c] = (g.in && c < C) ? dL_dF[(size_t)c * HW + g.pix] : 0.0f;
    s_g[lane * CG + c] = gp[c];
    if (feature_bg && c < C) bgdot = bgdot + feature_bg[c] * gp[c];
  }
  float Tr = tf, S = 0.0f;
  const float nTfin = -tf;
  const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;
  const int fj = lane & 31, fh = lane >> 5;

  // the round that ends at position ce (exclusive) starts at round_start(ce); ce = 0: no round, its loads re-read position 0
  auto round_start = [](uint32_t ce) { return ce > (uint32_t)ROUND ? ce - ROUND : 0u; };
  Gather ga(splat, list, g);
  ga.load_id(round_start(maxn)); ga.load_rec(); ga.load_id(round_start(round_start(maxn)));
  uint32_t cend = maxn;
  while (cend > 0) {
    const uint32_t cstart = round_start(cend);
    const int n = (int)(cend - cstart);
    // (its barriers also order s_g's writes)
    const int ns = stage_round<CG>(s_rec, s_id, s_f, ga, n, cstart, round_start(round_start(cstart)), C, cull, g, features);
    for (int c1 = ns; c1 > 0; c1 -= FLUSH) {
      const int c0 = c1 > FLUSH ? c1 - FLUSH : 0;   // the chunk: staged records c0 .. c1 - 1
      uint32_t touched = 0;              // wave-uniform: records of the chunk some pixel of the quarter blended
      for (int j = c1 - 1; j >= c0; --j) {
        const float4 a = s_rec[j * 2 + 0], b = s_rec[j * 2 + 1];
        float dx, dy;
        const float pw = blend_power(a.x, a.y, a.z, a.w, b.x, pxf, pyf, dx, dy);
        const float thr = cull ? b.y : -__builtin_huge_valf();
        const bool need = __float_as_uint(b.w) < lastn && pw >= thr;
        if (__ballot(need) == 0ull) continue;
        float adec;
        const float g0 = blend_exp_backward<EXP_MODE>(pw, b.z, adec);
        const float a0 = fminf(0.99f, b.z * g0);
        const bool live = need && !(pw > 0.0f) && !(adec < ALPHA_FLOOR);
        if (__ballot(live) == 0ull) continue;
        touched |= 1u << (j - c0);
        const float G = live ? g0 : 0.0f, alpha = live ? a0 : 0.0f;
        const float om = 1.0f - alpha;
        float inv = __builtin_amdgcn_rcpf(om);
        inv = __builtin_fmaf(inv, __builtin_fmaf(-om, inv, 1.0f), inv);
        Tr = Tr * inv;
        const float* f = s_f + j * CG;
        float gf = 0.0f;
#pragma unroll
        for (int c = 0; c < CG; ++c) gf = __builtin_fmaf(gp[c], f[c], gf);
        const float d = gf - S;
        S = __builtin_fmaf(alpha, d, S);
        const float dL_dalpha = __builtin_fmaf(nTfin * inv, bgdot, d * Tr);
        s_w[(j - c0) * WPAD + lane] = alpha * Tr;
        s_q[(j - c0) * WPAD + lane] = live ? G * dL_dalpha : 0.0f;
      }
      __syncthreads();
      const bool mine = fj < c1 - c0 && ((touched >> fj) & 1u);
      const int rj = min(c0 + fj, ROUND - 1);   // the lane's record in the staging area (clamped: an idle lane reads, never uses)
      // the record's dL/dfeatures row, channels fh * CH .. : sum over the 64 pixels, in pixel order
      float acc[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
      if (mine) {
        // (the pixel loops stay rolled: fully unrolled, the small channel groups hoist every LDS read and spill)
#pragma unroll 4
        for (int p = 0; p < 64; ++p) {
          const float w = s_w[fj * WPAD + p];
          const float* gq = s_g + p * CG + fh * CH;
#pragma unroll
          for (int c = 0; c < CH; ++c) acc[c] = __builtin_fmaf(w, gq[c], acc[c]);
        }
      }
      {
        // the six geometry sums of the record over the pixels fh * 32 .. (every lane runs the exchange; an idle lane carries zeros)
        const float4 a = s_rec[rj * 2 + 0], b = s_rec[rj * 2 + 1];
        float s3 = 0.0f, s4 = 0.0f, s5 = 0.0f, swx = 0.0f, swy = 0.0f, sop = 0.0f;
        if (mine) {
#pragma unroll 4
          for (int pp = 0; pp < 32; ++pp) {
            const int p = fh * 32 + pp;
            const float q = s_q[fj * WPAD + p];
            const float dx = a.x - (float)(g.qx0 + (p & 7)), dy = a.y - (float)(g.qy0 + (p >> 3));
            const float wx = q * dx, wy = q * dy;
            s3 = __builtin_fmaf(wx, dx, s3); s4 = __builtin_fmaf(wx, dy, s4); s5 = __builtin_fmaf(wy, dy, s5);
            swx += wx; swy += wy; sop += q;
          }
        }
        s3 += __shfl_xor(s3, 32, 64); s4 += __shfl_xor(s4, 32, 64); s5 += __shfl_xor(s5, 32, 64);
        swx += __shfl_xor(swx, 32, 64); swy += __shfl_xor(swy, 32, 64); sop += __shfl_xor(sop, 32, 64);
        if (mine) {
          float* rec = grad_acc + GGD_ACC_FLOATS * (size_t)s_id[rj];
          // half 0: conic A B C; half 1: opacity, mean x, mean y -- scaled as the colour backward's flush scales them
          const float v0 = fh == 0 ? s3 : sop, v1 = fh == 0 ? s4 : swx, v2 = fh == 0 ? s5 : swy;
          const int k0 = fh == 0 ? GGD_ACC_CONIC : GGD_ACC_OPACITY;
          atomicAdd(rec + k0 + 0, bwd_scale(k0 + 0, v0, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
          atomicAdd(rec + k0 + 1, bwd_scale(k0 + 1, v1, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
          atomicAdd(rec + k0 + 2, bwd_scale(k0 + 2, v2, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
        }
      }
      // the rows go out through LDS, (record, channel) pairs over the lanes with the channel fastest: a record's C atomics form one
      // span of 4 C bytes in one instruction, as the colour backward's flush forms its 36-byte spans (a lane per record and a
      // channel per instruction puts 64 cache lines into every atomic instruction)
      __syncthreads();                   // s_w is consumed
      if (mine) {
#pragma unroll
        for (int c = 0; c < CH; ++c) s_w[fj * CG + fh * CH + c] = acc[c];
      }
      __syncthreads();
      for (int t = lane; t < (c1 - c0) * CG; t += 64) {
        const int r = t / CG, c = t - r * CG;
        if (((touched >> r) & 1u) && c < C) atomicAdd(dL_dfeatures + (size_t)s_id[c0 + r] * C + c, s_w[t]);
      }
      __syncthreads();                   // the chunk's parked values are consumed before the next chunk's are written
    }
    cend = cstart;
  }
}

// channel-group width of C: 4, 8, 16, 32 -> 0 .. 3
inline int channel_group(int C) { return C <= 4 ? 0 : (C <= 8 ? 1 : (C <= 16 ? 2 : 3)); }

}  // namespace

int ggd_launch_features_forward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                const uint32_t* list, const uint32_t* ranges, uint32_t R, const uint32_t* n_contrib,
                                const float* features, int C, const float* feature_bg, float* out) {
  const QuarterLaunch q = quarter_launch(ctx, prm, true);
  if (q.T == 0) return GGD_OK;
  ggd_dispatch<3>(q.em, [&](auto e) {
    ggd_dispatch<4>(channel_group(C), [&](auto cg) {
      hipLaunchKernelGGL((features_forward_kernel<decltype(e)::value, (4 << decltype(cg)::value)>), dim3(4 * q.T), dim3(64), 0, s,
                         prm.width, prm.height, q.gx, q.T, C, q.cull, splat, list, ranges, R, n_contrib, features, feature_bg, out);
    });
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

int ggd_launch_features_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                 const uint32_t* list, const uint32_t* ranges, uint32_t R, const float* final_T,
                                 const uint32_t* n_contrib, const float* features, int C, const float* feature_bg,
                                 const float* dL_dF, float* grad_acc, float* dL_dfeatures) {
  const QuarterLaunch q = quarter_launch(ctx, prm, false);
  if (q.T == 0) return GGD_OK;
  ggd_dispatch<4>(q.em, [&](auto e) {
    ggd_dispatch<4>(channel_group(C), [&](auto cg) {
      hipLaunchKernelGGL((features_backward_kernel<decltype(e)::value, (4 << decltype(cg)::value)>), dim3(4 * q.T), dim3(64), 0, s,
                         prm.width, prm.height, q.gx, q.T, C, q.cull, splat, list, ranges, R, final_T, n_contrib, features,
                         feature_bg, dL_dF, grad_acc, dL_dfeatures);
    });
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
