// ggd_distortion.hip -- the depth-distortion map over the contributors of a finished colour render (ggd_forward_distortion /
// ggd_backward_distortion).
//
//   D = sum_i sum_j w_i w_j |z_i - z_j| = 2 sum_k w_k (z_k A_{k-1} - B_{k-1})      w = alpha T,  A_k = sum_{j<=k} w_j,  B_k = sum_{j<=k} w_j z_j
//
// (the second form because a tile's list is sorted by the depth key, a monotone image of z).  The contributors, their alpha and
// their T are the colour pass's: both kernels are the quarter walk of ggd_quarter_walk.h, as the feature blend is -- the tile's
// sorted list bounded per pixel by the stored n_contrib, alpha recomputed with the colour kernels' own expressions
// (ggd_blend_math.h); z_k is the fp32 the preprocess kernel stored in depth_keys, gathered and staged beside the record.
//
// Backward, with g = dL/dD of the pixel and S^A_k = A - A_k, S^B_k = B - B_k the sums BEHIND record k:
//   dD/dz_k = 2 w_k (A_{k-1} - S^A_k)                                          -> accumulator slot GGD_ACC_DEPTH
//   dD/dw_k = 2 u_k,   u_k = (z_k A_{k-1} - B_{k-1}) + (S^B_k - z_k S^A_k)
// and for dL/dalpha_k the map is a one-channel blend of the per-(pixel, record) values c_k = 2 g u_k without a background: the
// colour backward's recurrence rec <- alpha_k c_k + (1 - alpha_k) rec, dL/dalpha_k = (c_k - rec_behind) T_k, then bwd_scale into
// GGD_ACC_CONIC / _OPACITY / _MEAN2D.  The walk is back to front, so S^A, S^B grow with it; the prefixes are A - S^A_k - w_k with
// the pixel's totals A, B from a forward pre-pass inside the same kernel -- the forward kernel's own loop (walk_totals), hence the
// forward's numbers bit for bit.  (1 - final_T is A only up to the rounding of the transmittance product, which is the whole of A
// on a faint pixel; and no stored plane holds B.)
#include "ggd_common.h"

namespace {

#include "ggd_blend_math.h"
#include "ggd_quarter_walk.h"

// the record gather with the Gaussian's depth beside it
struct DepthGather {
  Gather g; const uint32_t* depth_keys;
  uint32_t z = 0;                        // fp32 bits of the view-space depth of the record in g.r0 .. r2
  __device__ __forceinline__ void load_id(uint32_t pos0) { g.load_id(pos0); }
  __device__ __forceinline__ void load_rec() { g.load_rec(); z = depth_keys[g.id_cur]; }
};

// One round's records (stage_cull) and their z into LDS; the next round's records and the ids of the one after are requested at
// once.  Returns the number of staged records (wave-uniform).
__device__ __forceinline__ int stage_records(float4* s_rec, float* s_z, uint32_t* s_id, DepthGather& ga, int n, uint32_t pos0,
                                             uint32_t pos_after_next, int cull, const QuarterGeom& g) {
  const int ns = stage_cull(s_rec, s_id, ga.g, g, n, pos0, cull, [&](int slot) { s_z[slot] = __uint_as_float(ga.z); });
  ga.load_rec();
  ga.load_id(pos_after_next);
  __syncthreads();
  return ns;
}

// The forward walk of the lane's pixel: A = sum w, B = sum w z, D = sum_k w_k (z_k A_{k-1} - B_{k-1}) (half the map's value).
// EXP_MODE: the colour forward's (0, 1, 2).
template <int EXP_MODE>
__device__ __forceinline__ void walk_totals(float4* s_rec, float* s_z, uint32_t* s_id, const QuarterGeom& g, int cull,
                                            const ggd_splat* __restrict__ splat, const uint32_t* __restrict__ list,
                                            const uint32_t* __restrict__ depth_keys, float& A, float& B, float& D) {
  A = 0.0f; B = 0.0f; D = 0.0f;
  DepthGather ga = {Gather(splat, list, g), depth_keys};
  walk_front<EXP_MODE>(
      s_rec, g, cull, ga,
      [&](int n, uint32_t pos0, uint32_t pos_after_next) {
        return stage_records(s_rec, s_z, s_id, ga, n, pos0, pos_after_next, cull, g);
      },
      [&](int j, const PairForward& p) {
        const float z = s_z[j];
        D = __builtin_fmaf(p.w, __builtin_fmaf(z, A, -B), D);
        A = A + p.w;
        B = __builtin_fmaf(p.w, z, B);
      });
}

// ---- forward -------------------------------------------------------------------------------------------------------------
template <int EXP_MODE>
__global__ __launch_bounds__(64) void distortion_forward_kernel(int W, int H, int gx, int T, int cull,
                                                                const ggd_splat* __restrict__ splat,
                                                                const uint32_t* __restrict__ list,
                                                                const uint32_t* __restrict__ ranges, uint32_t R,
                                                                const uint32_t* __restrict__ n_contrib,
                                                                const uint32_t* __restrict__ depth_keys,
                                                                float* __restrict__ out) {
  __shared__ float4 s_rec[ROUND * 2];
  __shared__ float s_z[ROUND];
  __shared__ uint32_t s_id[ROUND];
  const QuarterGeom g((int)blockIdx.x, W, H, gx, T, ranges, R, n_contrib);
  float A, B, D;
  walk_totals<EXP_MODE>(s_rec, s_z, s_id, g, cull, splat, list, depth_keys, A, B, D);
  if (g.in) out[g.pix] = 2.0f * D;
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// EXP_MODE: the colour backward's (0 .. 3); the pre-pass runs the forward's exponential of that mode (the bare one for mode 3).
// Records are visited back to front from the quarter's deepest last contributor; a pixel that does not see a record gets
// alpha = G = 0, which makes every state update an exact no-op.  A round's staged records are taken in chunks of FLUSH = 32, from
// the back: the pixel lanes park q = G dL/dalpha and v = g dD/dz of every (record, pixel) pair of the chunk some pixel sees; then
// lane (j, h) = (lane & 31, lane >> 5) owns record j of the chunk and half h of the pixels of its seven sums, combined over the
// two halves with one cross-half exchange.
template <int EXP_MODE>
__global__ __launch_bounds__(64) void distortion_backward_kernel(int W, int H, int gx, int T, int cull,
                                                                 const ggd_splat* __restrict__ splat,
                                                                 const uint32_t* __restrict__ list,
                                                                 const uint32_t* __restrict__ ranges, uint32_t R,
                                                                 const float* __restrict__ final_T,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 const uint32_t* __restrict__ depth_keys,
                                                                 const float* __restrict__ dL_dD,
                                                                 float* __restrict__ grad_acc) {
  __shared__ float4 s_rec[ROUND * 2];
  __shared__ float s_z[ROUND];
  __shared__ uint32_t s_id[ROUND];
  __shared__ float s_q[FLUSH * WPAD];    // G dL/dalpha    of (record of the chunk, pixel)
  __shared__ float s_v[FLUSH * WPAD];    // g dD/dz        of (record of the chunk, pixel)
  const int lane = threadIdx.x;
  const QuarterGeom g((int)blockIdx.x, W, H, gx, T, ranges, R, n_contrib);
  const uint32_t lastn = g.lastn, maxn = g.maxn;
  if (maxn == 0) return;
  const float g2 = g.in ? 2.0f * dL_dD[g.pix] : 0.0f;
  if (__ballot(g2 != 0.0f) == 0ull) return;   // every term below carries the pixel's g
  float A, B, D;
  walk_totals<(EXP_MODE == 3 ? 1 : EXP_MODE)>(s_rec, s_z, s_id, g, cull, splat, list, depth_keys, A, B, D);

  const float pxf = (float)g.px, pyf = (float)g.py;
  float Tr = g.in ? final_T[g.pix] : 0.0f;
  float SA = 0.0f, SB = 0.0f, rec = 0.0f;   // sum w, sum w z and the composited c behind the record
  const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;
  const int fj = lane & 31, fh = lane >> 5;

  // the round that ends at position ce (exclusive) starts at round_start(ce); ce = 0: no round, its loads re-read position 0
  auto round_start = [](uint32_t ce) { return ce > (uint32_t)ROUND ? ce - ROUND : 0u; };
  DepthGather ga = {Gather(splat, list, g), depth_keys};
  ga.load_id(round_start(maxn)); ga.load_rec(); ga.load_id(round_start(round_start(maxn)));
  uint32_t cend = maxn;
  while (cend > 0) {
    const uint32_t cstart = round_start(cend);
    const int n = (int)(cend - cstart);
    const int ns = stage_records(s_rec, s_z, s_id, ga, n, cstart, round_start(round_start(cstart)), cull, g);
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
        Tr = Tr * inv;                   // T_k
        const float w = alpha * Tr;
        const float z = s_z[j];
        const float PA = (A - SA) - w;                          // A_{k-1}
        const float PB = __builtin_fmaf(-w, z, B - SB);         // B_{k-1}
        const float u = __builtin_fmaf(z, PA, -PB) + __builtin_fmaf(-z, SA, SB);
        const float d = __builtin_fmaf(g2, u, -rec);            // c_k - rec_behind
        rec = __builtin_fmaf(alpha, d, rec);
        s_q[(j - c0) * WPAD + lane] = G * (d * Tr);             // (G = 0 where the pixel does not see the record)
        s_v[(j - c0) * WPAD + lane] = (g2 * w) * (PA - SA);     // (w = 0 likewise)
        SA = SA + w;
        SB = __builtin_fmaf(w, z, SB);
      }
      __syncthreads();
      const bool mine = fj < c1 - c0 && ((touched >> fj) & 1u);
      const int rj = min(c0 + fj, ROUND - 1);   // the lane's record in the staging area (clamped: an idle lane reads, never uses)
      // the seven sums of the record over the pixels fh * 32 .. (every lane runs the exchange; an idle lane carries zeros)
      const float4 a = s_rec[rj * 2 + 0], b = s_rec[rj * 2 + 1];
      float s3 = 0.0f, s4 = 0.0f, s5 = 0.0f, swx = 0.0f, swy = 0.0f, sop = 0.0f, sz = 0.0f;
      if (mine) {
#pragma unroll 4
        for (int pp = 0; pp < 32; ++pp) {
          const int p = fh * 32 + pp;
          const float q = s_q[fj * WPAD + p];
          const float dx = a.x - (float)(g.qx0 + (p & 7)), dy = a.y - (float)(g.qy0 + (p >> 3));
          const float wx = q * dx, wy = q * dy;
          s3 = __builtin_fmaf(wx, dx, s3); s4 = __builtin_fmaf(wx, dy, s4); s5 = __builtin_fmaf(wy, dy, s5);
          swx += wx; swy += wy; sop += q;
          sz += s_v[fj * WPAD + p];
        }
      }
      s3 += __shfl_xor(s3, 32, 64); s4 += __shfl_xor(s4, 32, 64); s5 += __shfl_xor(s5, 32, 64);
      swx += __shfl_xor(swx, 32, 64); swy += __shfl_xor(swy, 32, 64); sop += __shfl_xor(sop, 32, 64);
      sz += __shfl_xor(sz, 32, 64);
      if (mine) {
        float* r = grad_acc + GGD_ACC_FLOATS * (size_t)s_id[rj];
        // half 0: conic A B C and z; half 1: opacity, mean x, mean y -- slots 0 .. 5 of a record are one 24-byte span per
        // instruction pair, scaled as the colour backward's flush scales them; the z slot lies behind the colour's three
        const float v0 = fh == 0 ? s3 : sop, v1 = fh == 0 ? s4 : swx, v2 = fh == 0 ? s5 : swy;
        const int k0 = fh == 0 ? GGD_ACC_CONIC : GGD_ACC_OPACITY;
        atomicAdd(r + k0 + 0, bwd_scale(k0 + 0, v0, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
        atomicAdd(r + k0 + 1, bwd_scale(k0 + 1, v1, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
        atomicAdd(r + k0 + 2, bwd_scale(k0 + 2, v2, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
        if (fh == 0) atomicAdd(r + GGD_ACC_DEPTH, sz);
      }
      __syncthreads();                   // the chunk's parked values are consumed before the next chunk's are written
    }
    cend = cstart;
  }
}

}  // namespace

int ggd_launch_distortion_forward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                  const uint32_t* list, const uint32_t* ranges, uint32_t R, const uint32_t* n_contrib,
                                  const uint32_t* depth_keys, float* out) {
  const QuarterLaunch q = quarter_launch(ctx, prm, true);
  if (q.T == 0) return GGD_OK;
  ggd_dispatch<3>(q.em, [&](auto e) {
    hipLaunchKernelGGL((distortion_forward_kernel<decltype(e)::value>), dim3(4 * q.T), dim3(64), 0, s, prm.width, prm.height, q.gx,
                       q.T, q.cull, splat, list, ranges, R, n_contrib, depth_keys, out);
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

int ggd_launch_distortion_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                                   const uint32_t* list, const uint32_t* ranges, uint32_t R, const float* final_T,
                                   const uint32_t* n_contrib, const uint32_t* depth_keys, const float* dL_dD, float* grad_acc) {
  const QuarterLaunch q = quarter_launch(ctx, prm, false);
  if (q.T == 0) return GGD_OK;
  ggd_dispatch<4>(q.em, [&](auto e) {
    hipLaunchKernelGGL((distortion_backward_kernel<decltype(e)::value>), dim3(4 * q.T), dim3(64), 0, s, prm.width, prm.height, q.gx,
                       q.T, q.cull, splat, list, ranges, R, final_T, n_contrib, depth_keys, dL_dD, grad_acc);
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
