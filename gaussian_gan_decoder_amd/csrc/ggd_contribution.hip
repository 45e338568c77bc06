// ggd_contribution.hip -- per-Gaussian contribution statistics of a finished colour render (ggd_contribution; DESIGN.md section
// 6zi): over every (pixel, record) pair the colour pass blended, with w = alpha T,
//
//   stats[id][0] += rint(w 2^24)           the summed blend weight, fixed point (GGD_CONTRIB_SCALE_LOG2 = 24)
//   stats[id][1] += 1                      the pixel count
//   stats[id][2]  = max(., bits(w))        the largest blend weight (w > 0: the bit pattern orders as the value)
//
// Forward only.  The walk is the feature forward's -- the quarter walk of ggd_quarter_walk.h (walk_front / pair_forward): one
// single-wave workgroup per 8x8 quarter, one pixel per lane, bounded per pixel by the stored n_contrib, the colour kernels' skip
// tests in the colour kernels' order -- so a pair is in or out exactly as it was in the colour, and its w is the colour's bits.
//
// What is this file's: the reduction over the quarter's pixels before memory is touched.  The pixel lanes park w of a round's staged
// records in LDS as [record][pixel] (row stride WPAD, as the backward kernels park theirs); behind the round lane = record forms its
// row's sum, count and max over the 64 pixels and issues three integer atomics on the record's 24-byte row -- at most one update of
// a row per (quarter, record), up to 64 lanes active per atomic instruction.  A row's sum over one quarter is below 64 * 2^24 < 2^30
// and is formed in 32 bits.  Integer atomics commute: the result is bit-identical from run to run and accumulates over frames in
// place.  A record no pixel of the quarter blended is neither read nor written.
#include "ggd_common.h"

namespace {

#include "ggd_blend_math.h"
#include "ggd_quarter_walk.h"

static_assert(GGD_CONTRIB_SCALE_LOG2 == 24, "the fixed-point scale is 2^24: w 2^24 < 2^24 is exact in fp32 and a quarter's sum fits 32 bits");

template <int EXP_MODE>
__global__ __launch_bounds__(64) void contribution_kernel(int W, int H, int gx, int T, int cull,
                                                          const ggd_splat* __restrict__ splat,
                                                          const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ ranges, uint32_t R,
                                                          const uint32_t* __restrict__ n_contrib,
                                                          unsigned long long* __restrict__ stats) {
  __shared__ float4 s_rec[ROUND * 2];
  __shared__ uint32_t s_id[ROUND];
  __shared__ float s_w[ROUND * WPAD];    // alpha T of (staged record of the round, pixel)
  const int lane = threadIdx.x;
  const QuarterGeom g((int)blockIdx.x, W, H, gx, T, ranges, R, n_contrib);
  if (g.maxn == 0) return;

  uint64_t touched = 0;                  // wave-uniform: staged records of the round some pixel of the quarter got a step of
  // the round's rows out: lane = record.  Called in front of the next round's staging (whose opening barrier sets its LDS writes
  // behind these reads) and behind the last round.
  auto flush = [&]() {
    if (touched == 0) return;
    __syncthreads();                     // the pixel lanes' parked weights
    if ((touched >> lane) & 1ull) {
      const float* row = s_w + lane * WPAD;
      uint32_t sum = 0, cnt = 0, mx = 0;
#pragma unroll 8
      for (int p = 0; p < 64; ++p) {
        const float w = row[p];
        sum += (uint32_t)rintf(w * 16777216.0f);
        cnt += w > 0.0f ? 1u : 0u;
        mx = max(mx, __float_as_uint(w));
      }
      if (cnt) {
        unsigned long long* r = stats + 3 * (size_t)s_id[lane];
        atomicAdd(r + 0, (unsigned long long)sum);
        atomicAdd(r + 1, (unsigned long long)cnt);
        atomicMax(r + 2, (unsigned long long)mx);
      }
    }
    touched = 0;
  };

  Gather ga(splat, list, g);
  walk_front<EXP_MODE>(
      s_rec, g, cull, ga,
      [&](int n, uint32_t pos0, uint32_t pos_after_next) {
        flush();
        const int ns = stage_cull(s_rec, s_id, ga, g, n, pos0, cull, [](int) {});
        ga.load_rec();
        ga.load_id(pos_after_next);
        __syncthreads();
        return ns;
      },
      [&](int j, const PairForward& p) {
        touched |= 1ull << j;
        s_w[j * WPAD + lane] = p.w;      // 0 where the pixel does not blend the record
      });
  flush();
}

}  // namespace

int ggd_launch_contribution(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat, const uint32_t* list,
                            const uint32_t* ranges, uint32_t R, const uint32_t* n_contrib, int64_t* stats) {
  const QuarterLaunch q = quarter_launch(ctx, prm, true);
  if (q.T == 0) return GGD_OK;
  ggd_dispatch<3>(q.em, [&](auto e) {
    hipLaunchKernelGGL((contribution_kernel<decltype(e)::value>), dim3(4 * q.T), dim3(64), 0, s, prm.width, prm.height, q.gx, q.T,
                       q.cull, splat, list, ranges, R, n_contrib, reinterpret_cast<unsigned long long*>(stats));
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
