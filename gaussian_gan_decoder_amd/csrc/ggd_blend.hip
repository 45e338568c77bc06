// ggd_blend.hip -- stages a9 (forward alpha blend) and a10 (backward blend) for gfx950.
//
// Replaces renderCUDA fwd/bwd inside `_C.rasterize_gaussians{,_backward}` (reached from
// gaussian_splatting/gaussian_renderer/__init__.py:167-175; algorithm restated in SURVEY.md 9.4 / 9.5).
//
// wave64 design (not the 16x16-thread block of the CUDA original):
//   * The unit of work is an 8x8 QUARTER of a 16x16 tile, one pixel per lane: forward = one single-wave workgroup per
//     quarter (the four quarters of a tile in consecutive dispatch slots of one XCD, so that they share its L2); backward =
//     four independent quarter waves (large grids) or four quarter waves in one workgroup that combine their per-record sums
//     in LDS (an explicit, non-default choice).  Why the smallest block: the VALU cost of a blended record is proportional to the
//     pixels a wave holds (packed fp32 brings no throughput on gfx950), while a record typically reaches less than half of
//     a block, so the smallest block culls finest and idles fewest lanes.  The wider blocks (16x8 with 2 pixels per lane,
//     16x16 with 4) were measured and removed: DESIGN.md section 4 has the figures, git history the code.
//   * A tile's depth-sorted list is consumed 64 records per round: lane j gathers record j (one 48-byte ggd_splat, three
//     16-byte loads).  The gather is a two-stage software pipeline -- the list entries of round k + 2 and the records of
//     round k + 1 are in flight while round k is blended.  The gathering lane tests its record against the wave's pixel
//     rectangle (axis-aligned box of {alpha >= 1/255}, then the exact maximum of `power` over the rectangle); only the
//     survivors are staged, compacted, in LDS, as loaded plus two in-place words.  The rectangle shrinks round by round
//     to the pixels that are still live (forward) / that can see the round (backward).
//   * Staged records are read back as LDS broadcasts in straight-line groups of 8.  Per record: a wave-level cull in the
//     power domain before any exp (one scalar branch), then a branch-free update in which every per-pixel condition is a
//     wave-uniform 64-bit lane mask in an SGPR pair (v_cmp -> SGPR, combined on the scalar unit) and every state change a VOP3
//     select on such a mask with a tied destination (inline asm: the compiler's VCC-form select costs 8.7 issue slots).
//   * No workgroup barrier in the forward or the quarter backward: "wave finished" is one wave-uniform ballot.
//   * Backward: the 9 per-Gaussian partial gradients are reduced over the wave with a transposed DPP butterfly folded by the
//     gfx950 lane-block swaps (no LDS round trip), parked in LDS per touched record, and flushed as (record, component) pairs
//     over the lanes -- component fastest, so a record's nine float atomics form one 36-byte span -- instead of one atomic
//     per (pixel, Gaussian, component).
#include <type_traits>

#include "ggd_common.h"

namespace {

// the alpha floor, the exp() variants (blend_exp, blend_exp_backward), the record-level pre-cull, ggd_block_to_tile and bwd_scale: shared with the feature
// blend (ggd_features.hip), one definition for both files
#include "ggd_blend_math.h"

// Wave <-> pixel mapping of the forward blend: a wave owns one 8x8 quarter of a 16x16 tile (2 x 2 quarters per tile), one
// pixel per lane, 8 lanes per row and 8 rows.  (16x8 blocks with two pixels per lane and 16x16 blocks with four were
// measured and removed: DESIGN.md section 4 has the figures, git history the code.)
struct QuarterGeom {
  int px0, py;
  uint32_t lo, hi;
  __device__ __forceinline__ QuarterGeom(int b, int gx, int T, const uint32_t* __restrict__ ranges, uint32_t capacity) {
    int tile, sub;
    ggd_block_to_tile(b, 4, T, tile, sub);
    const int tx = tile % gx, ty = tile / gx;
    const int lane = threadIdx.x;
    px0 = tx * 16 + (sub % 2) * 8 + lane % 8;
    py = ty * 16 + (sub / 2) * 8 + lane / 8;
    const uint2 r = reinterpret_cast<const uint2*>(ranges)[tile];
    lo = min(r.x, capacity); hi = min(r.y, capacity);  // capacity < R only in a speculative forward that is retried
  }
};

// Per-lane selects on WAVE-UNIFORM 64-bit lane masks held in SGPR pairs.  Measured on gfx950
// (scripts/probes/valu_rate_probe.hip): v_cndmask_b32 in its VOP2 form (mask in VCC) issues at 1/8.7 of the v_fma_f32
// rate, the VOP3 form with an SGPR-pair mask at 1/1.6 -- and hipcc picks the VOP2 form whenever the mask happens to
// live in VCC.  Going through these helpers pins the VOP3 form and ties destination = old value (no copies where the
// culled and the updated path of the record loop join).
__device__ __forceinline__ void sel_into(float& dst, float src, uint64_t mask) {
  asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(src), "s"(mask));
}
__device__ __forceinline__ void sel_into(uint32_t& dst, uint32_t src, uint64_t mask) {
  asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(src), "s"(mask));
}
__device__ __forceinline__ float sel_or_zero(float src, uint64_t mask) {
  float d;
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(d) : "v"(src), "s"(mask));
  return d;
}
// dst = mask ? src : dst, ordered after the computation of `after` (a value that still needs the OLD dst: keeps the
// scheduler from sinking that use below the select, which would force a copy of the old value)
__device__ __forceinline__ void sel_into_after(float& dst, float src, uint64_t mask, float after) {
  asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(src), "s"(mask), "v"(after));
}
// acc += a * b in place (v_fmac_f32; through asm so that the SLP vectoriser does not pair the three colour channels
// into v_pk_fma_f32 with register shuffles -- packed fp32 has no throughput advantage on gfx950)
__device__ __forceinline__ void fma_into(float& acc, float a, float b) {
  asm("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b));
}

// Forward blend.  Per staged record:
//   (1) the `power` value of the lane's pixel (operation order == the published form),
//   (2) CULL: if no pixel of the wave can reach alpha >= 1/255 -- tested in the power domain against a per-record
//       threshold ln(1/(255*opacity)) lowered by a safety margin, so the decision is exact w.r.t. the float alpha
//       test that follows -- the whole wave skips the record before any exp,
//   (3) the exact per-pixel tests and the blend update, branch-free: every condition is a wave-uniform 64-bit lane mask
//       (v_cmp -> SGPR pair, combined on the scalar unit), every state update one select on such a mask.
// A finished pixel gets x = +inf: its power becomes -inf/NaN and it drops out in (2) with no extra instructions.
// Cost model (issue slots in units of one v_fma_f32 = ~2.5 cycles of a SIMD with >= 3 issuing waves, measured by the probes
// under scripts/probes): plain VALU 1, packed fp32 1.85 (no throughput gain over two plain ops on gfx950), v_cmp / VOP3
// select / v_min 1.6, v_exp_f32 3.1.  The forward executes 8 VALU instructions for a staged record no pixel sees and 28
// for one some pixel sees; the kernel runs at ~0.85 of the VALU rate in its steady state and spends a third of its time
// in ramp and tail.
// LDS reads through an explicit address-space-3 pointer (plain vector types: HIP's float4 class does not bind there)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const v4f lds_cf4;
__device__ __forceinline__ float4 lds_read4(lds_cf4* p) { const v4f v = *p; return make_float4(v[0], v[1], v[2], v[3]); }

// AUX (the depth / alpha extension, ggd_forward_aux): the gathering lane also loads the Gaussian's view-space depth
// (depth_keys = the fp32 bits of z, the depth sort's key) and stages it in the record's twelfth word, which the plain blend
// does not use (the cull extent ey, dead once the pre-cull has run) -- the staging area keeps its 48 bytes per record.  Per
// record one more FMA under the colour's `upd` mask accumulates sum(alpha T z); the epilogue writes it and 1 - T.
template <int EXP_MODE, bool CULL, bool STATS, bool AUX = false>
__device__ __forceinline__ void blend_forward_block(int blk, float4* s_rec, int W, int H, int gx, int T,
                                                    const ggd_splat* __restrict__ splat,
                                                    const uint32_t* __restrict__ list,
                                                    const uint32_t* __restrict__ ranges, uint32_t capacity,
                                                    const float* __restrict__ bg,
                                                    float* __restrict__ out_color,
                                                    float* __restrict__ final_T,
                                                    uint32_t* __restrict__ n_contrib,
                                                    unsigned long long* __restrict__ stats,
                                                    const uint32_t* __restrict__ depth_keys,
                                                    float* __restrict__ out_depth,
                                                    float* __restrict__ out_alpha) {
#ifndef GGD_FWD_GRP
#define GGD_FWD_GRP 8
#endif
  constexpr int GRP = GGD_FWD_GRP;   // staged records per straight-line group
  const int lane = threadIdx.x;
  const QuarterGeom g(blk, gx, T, ranges, capacity);
  const bool row_in = g.py < H;
  float INF = __builtin_huge_valf();
  asm volatile("" : "+v"(INF));   // keep it in a VGPR (VOP3 selects take no 32-bit literal)
  uint32_t st_visited = 0, st_culled = 0, st_lanes = 0, st_pixels = 0, st_inloop = 0;  // wave-uniform debug counters (GGD stats)
  const uint64_t st_t0 = STATS ? wall_clock64() : 0ull;                // 100 MHz constant clock: the wave's residency
  float Tr = 1.0f, C[3] = {0.0f, 0.0f, 0.0f};   // the lane's pixel: transmittance, accumulated colour
  float D = 0.0f;                               // AUX: accumulated depth
  uint32_t last = 0;
  float px = (row_in && g.px0 < W) ? (float)g.px0 : INF;   // pixel x coordinate; +inf once the pixel is finished / outside the image
  const float pyf = (float)g.py;
  auto wave_alive = [&]() { return __ballot(px < INF) != 0ull; };

  // the wave's pixel rectangle (pixel centres), for the record-level pre-cull
  const float wx0 = (float)(g.px0 - lane % 8), wx1 = wx0 + 7.0f;
  const float wy0 = (float)(g.py - lane / 8), wy1 = wy0 + 7.0f;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  // ... shrunk, round by round, to the bounding rectangle of the pixels that are still LIVE:
  // a wave runs until its last pixel is finished, and towards the end most records reach the block but none of the few
  // pixels left -- each such record cost a whole-wave test in the blend loop instead of one lane of the pre-cull.  Exact:
  // a finished pixel ignores every record.
  float lx0 = wx0, lx1 = wx1, ly0 = wy0, ly1 = wy1;
  auto shrink_rect = [&]() {
    const uint64_t live = __ballot(px < INF);
    if (live != 0ull) {
      const int rmin = __builtin_ctzll(live) >> 3, rmax = (63 - __builtin_clzll(live)) >> 3;
      uint32_t m = (uint32_t)live | (uint32_t)(live >> 32);
      m |= m >> 16; m |= m >> 8; m &= 0xffu;
      const int cmin = __builtin_ctz(m), cmax = 31 - __builtin_clz(m);
      lx0 = wx0 + (float)cmin; lx1 = wx0 + (float)cmax;
      ly0 = wy0 + (float)rmin; ly1 = wy0 + (float)rmax;
    }
  };

  // staged record = the 48-byte ggd_splat as loaded, two words replaced in place (three 16-byte LDS words, read back as
  // broadcasts; the cull stage needs the first two only):
  //   q0 = {x, y, -A/2, -B}   q1 = {-C/2, power threshold, opacity, r}   q2 = {g, b, contributor index (1-based list
  //   position; replaces the cull extent ex), -}
  // No component moves between the three words: forming a new 4-register tuple from parts of two loaded ones made the
  // register allocator copy those parts right behind the loads, i.e. wait for them there.
  bool keep = false;
  // The gather is a two-stage software pipeline, each stage one round (64 list entries) ahead of its consumer: the list
  // entries of round k + 2 and the 48-byte records of round k + 1 are in flight while round k is blended, and nothing is
  // waited for until the values are needed at the top of the next round.  (With the cull arithmetic inside the fetch the
  // compiler had to wait for both dependent loads -- list entry, then record -- right where they were issued: two exposed
  // memory round trips per round.)
  uint32_t id_nxt = 0;
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0;   // x y hA nB | hC thr opacity r | g b ex ey
  uint32_t zk = 0;                                          // AUX: depth key of the record in r0..r2
  // (unconditional loads from clamped positions: a lane past the end of the list re-reads the last entry -- one cache
  // line for the whole wave -- and its record is never consumed; exec-masked loads made r0..r2 loop-carried merges that the
  // register allocator split with copies right behind the loads, i.e. waits)
  const uint32_t last_pos = g.hi - 1u;   // only used when g.hi > g.lo
  auto load_id = [&](uint32_t pos) { id_nxt = list[min(pos, last_pos)]; };
  auto load_rec = [&]() {
    const float4* p = reinterpret_cast<const float4*>(splat + id_nxt);
    r0 = p[0]; r1 = p[1]; r2 = p[2];
    if constexpr (AUX) zk = depth_keys[id_nxt];
  };
  auto consume = [&](uint32_t pos) {   // cull decision of the record in r0..r2, then its two in-place edits
    keep = false;
    if (pos < g.hi) {
      keep = CULL ? (record_box_hits(r0.x, r0.y, r2.z, r2.w, lx0, lx1, ly0, ly1) &&
                     record_reaches_block(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r2.z, lx0, lx1, ly0, ly1)) : true;
      if (!CULL) r1.y = -__builtin_huge_valf();
      r2.z = __uint_as_float(pos - g.lo + 1u);
      if constexpr (AUX) r2.w = __uint_as_float(zk);   // view-space depth (the key is its fp32 bits)
    }
  };
  if (g.hi <= g.lo || !wave_alive()) goto all_done;
  load_id(g.lo + lane);
  load_rec();
  load_id(g.lo + 64 + lane);
  for (uint32_t base = g.lo; base < g.hi; base += 64) {
    if (CULL) shrink_rect();
    consume(base + lane);          // the records requested one round ago
    __syncthreads();  // single-wave block: orders the previous round's LDS reads before this round's writes
    const uint64_t kept = __ballot(keep);
    if (keep) {  // compacted: only records whose box reaches this wave's pixels are staged
      const int slot = __popcll(kept & lt_mask);
      s_rec[slot * 3 + 0] = r0; s_rec[slot * 3 + 1] = r1; s_rec[slot * 3 + 2] = r2;
    }
    // the staged list is walked in groups of 8 of straight-line code: LDS addresses are immediates, there is no loop
    // counter, a record that no pixel of the wave sees costs one scalar branch, and so does the end of the list inside the
    // last group (padding that group with records nobody can see cost their cull tests: 1 % of the kernel).  The blend
    // state is updated in place by the tied-operand selects below, inside a wave-uniform `if` -- nothing is copied where
    // the culled and the updated path join.
    const int n = __popcll(kept), n8 = (n + GRP - 1) & ~(GRP - 1);
    if (STATS) {
      st_visited += min(64u, g.hi - base);
      st_culled += min(64u, g.hi - base) - (uint32_t)__popcll(kept);
    }
    load_rec();                    // next round's records (their list entries were requested one round ago)
    // (that round's first position, named HERE: it is the loop's own increment, and formed only at the bottom of the loop it
    // makes the compiler rotate the loop, which costs the instances without pre-cull two VGPRs)
    const uint32_t next = base + 64;
    load_id(next + 64 + lane);     // and the list entries of the round after it
    __syncthreads();
    for (int j0 = 0; j0 < n8; j0 += GRP) {
      if (!wave_alive()) goto all_done;
      // the group's LDS address, held in a VGPR the compiler cannot rematerialise: as a wave-uniform value it lives in an
      // SGPR and every ds_read whose destination overlapped the address register re-copied it (two v_mov per record:
      // 6 % of the issue slots of an update, 11 % of an in-loop cull)
      uint32_t ga = (uint32_t)(uintptr_t)(lds_cf4*)(s_rec + j0 * 3);
      asm volatile("" : "+v"(ga));
      lds_cf4* grp = (lds_cf4*)(uintptr_t)ga;
      // ALL twelve words of a record are requested one record ahead (round 5; round 4 prefetched the six words of the cull
      // test and fetched the other six after the test had passed, 3 instructions before their first use -- an exposed LDS
      // round trip per update, and since the exact rectangle pre-cull 95 % of the staged records are updates).  Inside a
      // group only: carried across the group boundary the prefetched record is live on the loop's nine exit edges in
      // alternating register sets, which the compiler reconciles with ~100 v_mov per group.
      float4 a_nx = lds_read4(grp), b_nx = lds_read4(grp + 1), c_nx = lds_read4(grp + 2);
#pragma unroll
      for (int jj = 0; jj < GRP; ++jj) {
        if (j0 + jj >= n) break;   // (scalar compare + branch: the last group of a round is usually not full)
        const float4 a = a_nx, b4 = b_nx, c = c_nx;
        // (the record's twelfth word is not used: left dead, the register allocator hands its VGPR out as a temporary while the
        // load is still in flight, and the write-after-write hazard puts a wait for the whole prefetch three instructions
        // behind its issue; AUX: it is the depth)
        asm volatile("" : : "v"(c.w));
        const float2 b01 = make_float2(b4.x, b4.y);
        if (jj < GRP - 1) {
          a_nx = lds_read4(grp + (jj + 1) * 3);
          b_nx = lds_read4(grp + (jj + 1) * 3 + 1);
          c_nx = lds_read4(grp + (jj + 1) * 3 + 2);
        }
        const float dy = a.y - pyf;
        const float nBdy = a.w * dy, hCdy2 = (b01.x * dy) * dy;
        const float dx = a.x - px;
        const float pw = __builtin_fmaf(__builtin_fmaf(a.z, dx, nBdy), dx, hCdy2);
        const uint64_t need = __ballot(pw >= b01.y);
        if (need == 0ull) { if (STATS && j0 + jj < n) { st_culled += 1; st_inloop += 1; } continue; }
        if (STATS) { st_pixels += (uint32_t)__popcll(need); st_lanes += (uint32_t)__popcll(need); }
        const float2 b23 = make_float2(b4.z, b4.w);                                                                   // opacity, r
        const uint32_t contributor = __float_as_uint(c.z);
        const float G = blend_exp<EXP_MODE>(pw);
        const float alpha = fminf(0.99f, G * b23.x);
        const uint64_t live = need & ~__ballot(pw > 0.0f) & ~__ballot(alpha < ALPHA_FLOOR);
        const float test_T = Tr * (1.0f - alpha);
        const uint64_t low = __ballot(test_T < 0.0001f);
        const uint64_t upd = live & ~low, stop = live & low;
        const float w = sel_or_zero(alpha * Tr, upd);
        fma_into(C[0], b23.y, w);
        fma_into(C[1], c.x, w);
        fma_into(C[2], c.y, w);
        if constexpr (AUX) fma_into(D, c.w, w);
        sel_into_after(Tr, test_T, upd, w);
        sel_into(last, contributor, upd);
        if (stop) sel_into(px, INF, stop);   // a pixel stops once: a scalar branch (SCC of the s_and above), not a select per update
      }
    }
  }
all_done:

  if (STATS && lane == 0 && stats[GGD_STATS_MODE] != 0ull) {
    // timeline mode: this wave's [start, end] on the 100 MHz constant clock and the list entries it gathered -- plain
    // stores to its own slot (the counters' same-address atomics stretch the kernel tenfold); frames with more quarter
    // waves than the buffer has slots (beyond 32 768 tiles) record the first GGD_STATS_MAX_WAVES only
    if (blk < GGD_STATS_MAX_WAVES) {
      unsigned long long* slot = stats + GGD_STATS_HEAD + 3ull * (unsigned)blk;
      slot[0] = st_t0; slot[1] = wall_clock64(); slot[2] = ((unsigned long long)(g.hi - g.lo) << 32) | st_visited;
    }
  } else if (STATS && lane == 0) {
    atomicAdd(stats + 0, (unsigned long long)st_visited);
    atomicAdd(stats + 1, (unsigned long long)st_culled);
    atomicAdd(stats + 2, (unsigned long long)st_lanes);
    atomicAdd(stats + 3, (unsigned long long)st_pixels);
    atomicAdd(stats + 4, (unsigned long long)(g.hi - g.lo));
    atomicAdd(stats + 5, (unsigned long long)st_inloop);
  }
  if (!row_in || g.px0 >= W) return;
  const size_t HW = (size_t)H * W;
  const size_t pix0 = (size_t)g.py * W + g.px0;
  if constexpr (AUX) {
    out_depth[pix0] = D;
    out_alpha[pix0] = 1.0f - Tr;
  }
  final_T[pix0] = Tr;
  n_contrib[pix0] = last;
  out_color[pix0] = C[0] + Tr * bg[0];
  out_color[HW + pix0] = C[1] + Tr * bg[1];
  out_color[2 * HW + pix0] = C[2] + Tr * bg[2];
}

// One 8x8 quarter per single-wave workgroup (the launch has 4 T workgroups; workgroup b -> (XCD, tile, quarter), see
// ggd_block_to_tile).  A PERSISTENT form -- as many workgroups as the device holds, each drawing (tile, quarter) tickets
// from atomic counters, next ticket requested before the current tile is started -- was built and measured in round 4
// (commit 1e08ef1, profiles/r04/persist_ab_*.txt): 413 us with one counter per XCD, 184 us with 64 counters per XCD, against
// 104 us for this one-shot launch at 1 M / 1024^2 (shell 260 vs 194, 100 k / 512^2 79 vs 25): the same waves take the same
// time per tile, but 3.8 instead of 5.4 of them are at work per SIMD -- a ticket is a returning atomic's round trip through
// memory, the hardware dispatcher back-fills a finished wave's slot without one.  Removed again.
// AUX: the same blend with the depth / alpha planes (blend_forward_block); depth_keys, out_depth and out_alpha are NULL, and
// never read, in a plain frame.
template <int EXP_MODE, bool CULL, bool STATS, bool AUX = false>
__global__ __launch_bounds__(64) void blend_forward_kernel(int W, int H, int gx, int T,
                                                           const ggd_splat* __restrict__ splat,
                                                           const uint32_t* __restrict__ list,
                                                           const uint32_t* __restrict__ ranges, uint32_t capacity,
                                                           const float* __restrict__ bg,
                                                           float* __restrict__ out_color,
                                                           float* __restrict__ final_T,
                                                           uint32_t* __restrict__ n_contrib,
                                                           unsigned long long* __restrict__ stats,
                                                           const uint32_t* __restrict__ depth_keys,
                                                           float* __restrict__ out_depth,
                                                           float* __restrict__ out_alpha) {
  __shared__ float4 s_rec[64 * 3];
  blend_forward_block<EXP_MODE, CULL, STATS, AUX>((int)blockIdx.x, s_rec, W, H, gx, T, splat, list, ranges, capacity,
                                                           bg, out_color, final_T, n_contrib, stats, depth_keys, out_depth,
                                                           out_alpha);
}

// Backward blend: the per-record update of ONE pixel, shared by the two kernel forms below.  Records are visited back to
// front; the body is SELECT-FREE: a pixel that does not see the record (culled, beyond its n_contrib, alpha < 1/255) gets
// alpha = G = 0, which makes every state update an exact no-op (T / (1 - 0) = T, acc + 0 * (c - acc) = acc), so no per-pixel
// branches or selects on the recurrence state are needed.  1/(1 - alpha) is one v_rcp + one Newton step.
//   * The colour behind the record is folded in RIGHT AFTER its use: the published form keeps (last_alpha, last_color) and
//     folds one record late, accum = la * lc + (1 - la) * accum -- 17 instructions per update; with d = c - accum (needed for
//     dL/dalpha anyway) the same value is accum + alpha * d: 9 instructions and two words less state per pixel.
//   * The mean gradient leaves the pixel loop as the two sums  sum(dL/dalpha * G * dx), sum(dL/dalpha * G * dy); the conic's
//     2 x 2 matrix, the opacity, the -1/2 and the 0.5 W / 0.5 H of the pixel-to-NDC map are applied once per (record,
//     component) by the flush, not per pixel.
struct BwdPixel { float T, nTfin, bgdot, acc[3], gpx[3]; };
// AUX (depth / alpha extension): the depth is a fourth channel with background 0 (accD = the depth composited behind the
// record, gD = dL/ddepth of the pixel); dL/dalpha of the pixel is folded into bgdot (bwd_pixel_init)
struct BwdPixelAux : BwdPixel { float accD, gD; };
// The pixel's state at the back of its list (`in`: the pixel lies inside the image); returns the 1-based list position of its
// last contributor.  AUX: alpha = 1 - T_final, so dL/dT_final = bg . dL/dpix - dL/dalpha, folded into bgdot once (NULL
// gradients are taken as zero)
template <bool AUX, typename Pix>
__device__ __forceinline__ uint32_t bwd_pixel_init(Pix& st, bool in, size_t pix0, size_t HW, const float* __restrict__ bg,
                                                   const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                                                   const float* __restrict__ dL_dpix, const float* __restrict__ dL_ddepth,
                                                   const float* __restrict__ dL_dalpha) {
  const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];
  const float tf = in ? final_T[pix0] : 0.0f;
  const uint32_t lastn = in ? n_contrib[pix0] : 0u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) { st.gpx[ch] = in ? dL_dpix[ch * HW + pix0] : 0.0f; st.acc[ch] = 0.0f; }
  st.bgdot = (bg0 * st.gpx[0] + bg1 * st.gpx[1]) + bg2 * st.gpx[2];
  if constexpr (AUX) {
    st.accD = 0.0f;
    st.gD = (in && dL_ddepth) ? dL_ddepth[pix0] : 0.0f;
    st.bgdot = st.bgdot - ((in && dL_dalpha) ? dL_dalpha[pix0] : 0.0f);
  }
  st.T = tf; st.nTfin = -tf;
  return lastn;
}

// Lanes that hold a result of wave_reduce_swap (is_writer: lanes 0,4,8,12 | 32,36,40,44, lane 1 the opacity sum, AUX: lane 33
// the depth sum) and the word of the accumulator record it belongs to: reduction output index (colour r g b | conic A B C |
// mean sums x y | opacity | AUX: depth) -> slot in the record's order (conic A B C | opacity | mean x y | colour r g b | depth)
// ABS (absgrad extension): lanes 6 and 38 hold the two absolute mean sums; they have no accumulator-order place below slot
// GGD_ACC_ABS that every instance shares, so the value returned for them is their COLUMN in the parked row, right after the
// other sums (9, 10; AUX: 10, 11) -- the flush maps it to GGD_ACC_ABS, GGD_ACC_ABS + 1
template <bool AUX, bool ABS = false>
__device__ __forceinline__ int bwd_writer_comp(int lane, bool& is_writer) {
  is_writer = (lane & 19) == 0 || lane == 1 || (AUX && lane == 33) || (ABS && (lane & 31) == 6);
  if (ABS && (lane & 31) == 6) return 9 + (AUX ? 1 : 0) + (lane >> 5);
  const int val = lane == 1 ? 8 : ((AUX && lane == 33) ? 9 : 4 * (lane >> 5) + (((lane >> 2) & 1) << 1) + ((lane >> 3) & 1));
  return val < 3 ? GGD_ACC_COLOR + val
       : (val < 6 ? GGD_ACC_CONIC + (val - 3)
       : (val < 8 ? GGD_ACC_MEAN2D + (val - 6) : ((AUX && val == 9) ? GGD_ACC_DEPTH : GGD_ACC_OPACITY)));
}

// The list is walked back to front in rounds of at most 64 entries: first position of the round that ends at `ce` (exclusive,
// ce > lo = the list's first position)
__device__ __forceinline__ uint32_t bwd_round_start(uint32_t ce, uint32_t lo) { return (ce - lo > 64u) ? ce - 64u : lo; }

// The staged list is walked in groups of 8: slots nk .. n8 - 1 are filled with a record nobody sees (power threshold +inf)
__device__ __forceinline__ void bwd_stage_padding(float4* rec, int lane, int nk, int n8) {
  if (lane >= nk && lane < n8) {
    rec[lane * 3 + 0] = make_float4(0, 0, 0, 0);
    rec[lane * 3 + 1] = make_float4(0, __builtin_huge_valf(), 0, 0);
  }
}

// ABS (absgrad extension): sabs[0..1] = this pixel's |2 hA wx + nB wy|, |2 hC wy + nB wx| -- the expressions bwd_scale applies to
// the REDUCED sums, evaluated per pixel, because the absolute value has to be taken before the sum over the pixels (the
// non-negative factors op * 0.5 W, op * 0.5 H stay with the flush).  A pixel that does not see the record has wx = wy = 0.
template <int EXP_MODE, bool AUX = false, bool ABS = false, typename Pix = BwdPixel>
__device__ __forceinline__ uint64_t bwd_update(Pix& st, float pw, float dx, float dy, uint64_t need, float opacity,
                                               const float (&col)[3], float (&s)[8], float& sop, float z = 0.0f,
                                               float* sz = nullptr, float hA = 0.0f, float nB = 0.0f, float hC = 0.0f,
                                               float* sabs = nullptr) {
  // (mode 3, the default pairing: the CONTRIBUTION DECISION alpha >= 1/255 is taken on the forward's own number -- a record within a
  // few ulp of the floor is then in or out in both passes, and the transmittance replayed by T / (1 - alpha) stays consistent
  // with the saved final_T (decided on the accurate value, the two passes could disagree on such a record, 0.4 %
  // on everything in front of it in that pixel) -- while the VALUES use the compensated exponential: blend_exp_backward)
  float adec;
  const float g0 = blend_exp_backward<EXP_MODE>(pw, opacity, adec);
  const float a0 = fminf(0.99f, opacity * g0);
  const uint64_t live = need & ~__ballot(pw > 0.0f) & ~__ballot(adec < ALPHA_FLOOR);
  const float G = sel_or_zero(g0, live), alpha = sel_or_zero(a0, live);
  const float om = 1.0f - alpha;
  float inv = __builtin_amdgcn_rcpf(om);
  inv = __builtin_fmaf(inv, __builtin_fmaf(-om, inv, 1.0f), inv);
  st.T = st.T * inv;
  const float dchannel_dcolor = alpha * st.T;
  float dL_dalpha = 0.0f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float d = col[ch] - st.acc[ch];
    dL_dalpha = __builtin_fmaf(d, st.gpx[ch], dL_dalpha);
    fma_into(st.acc[ch], alpha, d);                       // in place: the culled path carries no copy
    s[ch] = dchannel_dcolor * st.gpx[ch];
  }
  if constexpr (AUX) {
    const float d = z - st.accD;
    dL_dalpha = __builtin_fmaf(d, st.gD, dL_dalpha);
    fma_into(st.accD, alpha, d);
    *sz = dchannel_dcolor * st.gD;
  }
  dL_dalpha = __builtin_fmaf(st.nTfin * inv, st.bgdot, dL_dalpha * st.T);
  const float wx = (G * dx) * dL_dalpha, wy = (G * dy) * dL_dalpha;
  s[3] = wx * dx;
  s[4] = wx * dy;
  s[5] = wy * dy;
  s[6] = wx;
  s[7] = wy;
  sop = G * dL_dalpha;
  if constexpr (ABS) {
    sabs[0] = __builtin_fabsf(__builtin_fmaf(2.0f * hA, wx, nB * wy));
    sabs[1] = __builtin_fabsf(__builtin_fmaf(2.0f * hC, wy, nB * wx));
  }
  return live;
}

// Nine wave sums with no LDS round trip: the eight of wave_reduce8_transposed plus a ninth that takes four all-lane DPP
// steps inside its row, then rides in the redundant lanes of the first register (after the quad steps the four lanes of
// a bank hold the same value; lane 4b + 1 of every bank is replaced by the ninth value's row sum).  The four rows are
// folded with the gfx950 lane-block swaps: v_permlane32_swap(x0, x1) leaves {x0 rows 0,1 | x1 rows 0,1} and
// {x0 rows 2,3 | x1 rows 2,3}, whose sum holds x0's values in lanes 0-31 and x1's in lanes 32-63 (two rows each);
// v_permlane16_swap of that sum with a copy of itself pairs the remaining two rows.  Result per lane l:
//   (l & 3) != 1:  value 4 * (l >> 5) + {0, 2, 1, 3}[(l >> 2) & 3]     l < 32 and (l & 3) == 1:  the ninth value
// TENTH (AUX: the depth sum): a tenth value takes the ninth's four in-row steps and rides in the redundant lanes 4b + 1 of the
// OTHER folded register (v[4]): after the two swaps lanes 32 <= l < 64 with (l & 3) == 1 hold it.
// ABS (absgrad extension: the two absolute mean sums): an eleventh and a twelfth value take the same four in-row steps and ride
// in the NEXT redundant lane, 4b + 2, of the two folded registers (eleventh: v[0], twelfth: v[4]): after the swaps lanes l < 32
// with (l & 3) == 2 hold the eleventh, lanes 32 <= l < 64 with (l & 3) == 2 the twelfth.  Their DPP steps follow the ninth's
// (tenth's) in each group, so every value's step is at least as far from the write it reads as the ninth's is.
// The text of the four forms is assembled from the same pieces: ONLY10(x) is x in the forms with a tenth value and nothing in
// the others, ONLYABS(x) likewise for the eleventh and twelfth.
#define GGD_RED_ROWSUM(r, ctl) "v_add_f32_dpp " r ", " r ", " r " " ctl " row_mask:0xf bank_mask:0xf\n\t"
#define GGD_RED_KEEP(x) x
#define GGD_RED_DROP(x)
#define GGD_RED_TEXT(ONLY10, ONLYABS)                                                                \
      "s_nop 1\n\t"                                                                           \
      "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                     \
      "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                     \
      "v_add_f32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                     \
      "v_add_f32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"                     \
      "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                     \
      "v_add_f32_dpp %2, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                     \
      "v_add_f32_dpp %4, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                     \
      "v_add_f32_dpp %6, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                     \
      GGD_RED_ROWSUM("%[ninth]", "row_ror:8") ONLY10(GGD_RED_ROWSUM("%[tenth]", "row_ror:8"))  \
      ONLYABS(GGD_RED_ROWSUM("%[absx]", "row_ror:8") GGD_RED_ROWSUM("%[absy]", "row_ror:8"))                      \
      "s_nop 0\n\t"                                                                           \
      "v_add_f32_dpp %0, %0, %0 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"                     \
      "v_add_f32_dpp %4, %4, %4 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"                     \
      GGD_RED_ROWSUM("%[ninth]", "row_ror:4") ONLY10(GGD_RED_ROWSUM("%[tenth]", "row_ror:4"))  \
      ONLYABS(GGD_RED_ROWSUM("%[absx]", "row_ror:4") GGD_RED_ROWSUM("%[absy]", "row_ror:4"))                      \
      "v_add_f32_dpp %0, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"                     \
      "v_add_f32_dpp %4, %6, %6 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"                     \
      "s_nop 1\n\t"                                                                           \
      GGD_RED_ROWSUM("%0", "quad_perm:[2,3,0,1]") GGD_RED_ROWSUM("%4", "quad_perm:[2,3,0,1]")  \
      GGD_RED_ROWSUM("%[ninth]", "quad_perm:[2,3,0,1]") ONLY10(GGD_RED_ROWSUM("%[tenth]", "quad_perm:[2,3,0,1]")) \
      ONLYABS(GGD_RED_ROWSUM("%[absx]", "quad_perm:[2,3,0,1]") GGD_RED_ROWSUM("%[absy]", "quad_perm:[2,3,0,1]"))  \
      "s_nop 0\n\t"                                                                           \
      GGD_RED_ROWSUM("%0", "quad_perm:[1,0,3,2]") GGD_RED_ROWSUM("%4", "quad_perm:[1,0,3,2]")  \
      GGD_RED_ROWSUM("%[ninth]", "quad_perm:[1,0,3,2]") ONLY10(GGD_RED_ROWSUM("%[tenth]", "quad_perm:[1,0,3,2]")) \
      ONLYABS(GGD_RED_ROWSUM("%[absx]", "quad_perm:[1,0,3,2]") GGD_RED_ROWSUM("%[absy]", "quad_perm:[1,0,3,2]"))  \
      "s_nop 1\n\t"                                                                           \
      "v_cndmask_b32_e64 %0, %0, %[ninth], %[mask]\n\t"                                       \
      ONLY10("v_cndmask_b32_e64 %4, %4, %[tenth], %[mask]\n\t")                               \
      ONLYABS("v_cndmask_b32_e64 %0, %0, %[absx], %[mask2]\n\t")                              \
      ONLYABS("v_cndmask_b32_e64 %4, %4, %[absy], %[mask2]\n\t")                              \
      "s_nop 1\n\t"                                                                           \
      "v_permlane32_swap_b32 %0, %4\n\t"                                                      \
      "s_nop 1\n\t"                                                                           \
      "v_add_f32_e32 %0, %0, %4\n\t"                                                          \
      "v_mov_b32_e32 %4, %0\n\t"                                                              \
      "s_nop 1\n\t"                                                                           \
      "v_permlane16_swap_b32 %0, %4\n\t"                                                      \
      "s_nop 1\n\t"                                                                           \
      "v_add_f32_e32 %0, %0, %4"
template <bool TENTH, bool ABS = false>
__device__ __forceinline__ float wave_reduce_swap(float (&v)[8], float ninth, float tenth, float absx = 0.0f,
                                                  float absy = 0.0f) {
  const uint64_t ninth_lanes = 0x2222222222222222ull;   // lane 4b + 1 of every bank
  [[maybe_unused]] const uint64_t abs_lanes = 0x4444444444444444ull;     // lane 4b + 2 of every bank
  if constexpr (TENTH && ABS)
    asm volatile(GGD_RED_TEXT(GGD_RED_KEEP, GGD_RED_KEEP)
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                   [ninth] "+v"(ninth), [tenth] "+v"(tenth), [absx] "+v"(absx), [absy] "+v"(absy)
                 : [mask] "s"(ninth_lanes), [mask2] "s"(abs_lanes));
  else if constexpr (ABS)
    asm volatile(GGD_RED_TEXT(GGD_RED_DROP, GGD_RED_KEEP)
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                   [ninth] "+v"(ninth), [absx] "+v"(absx), [absy] "+v"(absy)
                 : [mask] "s"(ninth_lanes), [mask2] "s"(abs_lanes));
  else if constexpr (TENTH)
    asm volatile(GGD_RED_TEXT(GGD_RED_KEEP, GGD_RED_DROP)
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                   [ninth] "+v"(ninth), [tenth] "+v"(tenth)
                 : [mask] "s"(ninth_lanes));
  else
    asm volatile(GGD_RED_TEXT(GGD_RED_DROP, GGD_RED_DROP)
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]),
                   [ninth] "+v"(ninth)
                 : [mask] "s"(ninth_lanes));
  return v[0];
}
#undef GGD_RED_TEXT
#undef GGD_RED_DROP
#undef GGD_RED_KEEP
#undef GGD_RED_ROWSUM

// ---- backward blend, tile form: the four 8x8 quarter waves of a tile in ONE workgroup --------------------------------
// (~60 VGPRs -> 8 waves per SIMD.)  Per round of 64 list entries every wave gathers the records itself (the other waves'
// copies hit L2), pre-culls them against its own rectangle and stages the survivors; the NEXT round's gather is issued
// before the current round is blended.  Staged records are walked back to front in groups of 8 as straight-line code (list
// padded with never-visible records, see the forward).  Per-record sums: transposed butterfly, parked in LDS per wave,
// combined over the waves by the flush -> one float atomic per (tile, Gaussian, component).
template <int EXP_MODE, bool CULL>
__global__ __launch_bounds__(256) void blend_backward_tile_kernel(
    int W, int H, int gx, int gy, const ggd_splat* __restrict__ splat, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ ranges, const float* __restrict__ bg, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dpix, float* __restrict__ grad_acc) {
  constexpr int NW = 4;
  __shared__ float4 s_rec[NW][64 * 3];
  // per-round results are double-buffered: a round's flush reads buffer `par` while early waves already fill the other
  // one, so a round costs ONE workgroup barrier (everybody finished the round), not two
  __shared__ float s_sum[2][NW][64][9];
  __shared__ uint32_t s_id[2][64];
  __shared__ float4 s_cop[2][64];      // hA, nB, hC, opacity of the round's records (the flush applies them)
  __shared__ uint32_t s_touch[2][NW][2];
  __shared__ uint32_t s_maxn[NW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int tile, sub_unused;
  ggd_block_to_tile((int)blockIdx.x, 1, gx * gy, tile, sub_unused);
  const int tx = tile % gx, ty = tile / gx;
  const int qx = wv & 1, qy = wv >> 1;
  const int px0 = tx * 16 + qx * 8 + (lane & 7), py = ty * 16 + qy * 8 + (lane >> 3);
  const uint2 rg = reinterpret_cast<const uint2*>(ranges)[tile];
  const bool in = py < H && px0 < W;
  const size_t HW = (size_t)H * W;
  const size_t pix0 = (size_t)py * W + px0;

  BwdPixel st;
  const float pxf = (float)px0, pyf = (float)py;
  const uint32_t lastn = bwd_pixel_init<false>(st, in, pix0, HW, bg, final_T, n_contrib, dL_dpix, nullptr, nullptr);
  uint32_t maxn = lastn;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, d, 64));
  if (lane == 0) s_maxn[wv] = maxn;
  __syncthreads();
  maxn = s_maxn[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) maxn = max(maxn, s_maxn[w]);   // workgroup-uniform: positions anyone in the tile contributed to
  if (maxn == 0) return;
  const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;
  const float wx0 = (float)(tx * 16 + qx * 8), wy0 = (float)(ty * 16 + qy * 8);   // this wave's pixel rectangle
  const float wx1 = wx0 + 7.0f, wy1 = wy0 + 7.0f;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  float4* rec = s_rec[wv];
  bool is_writer;
  const int writer_comp = bwd_writer_comp<false>(lane, is_writer);

  // staged = the record as loaded with three words replaced in place (no component changes its 16-byte word, see the forward):
  //   {x, y, hA, nB} {hC, power threshold, opacity, 0-based list position} {g, b, r, index inside the round}
  bool keep = false;
  // Two-stage software pipeline of the gather, as in the forward: while round k is blended the records of round k + 1
  // (the round in FRONT of it: the list is walked back to front) and the list entries of round k + 2 are in flight.
  uint32_t id_cur = 0, id_nxt = 0;     // Gaussian ids of the round whose records are in r0..r2 / of the round after it
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0;    // x y hA nB | hC thr opacity r | g b ex ey
  // (unconditional loads from clamped positions, see the forward; maxn > 0 here, so the list is not empty)
  auto load_id = [&](uint32_t ce) {    // the round that ends at list position ce (exclusive); ce <= rg.x: a dummy re-read
    const uint32_t cs = ce > rg.x ? bwd_round_start(ce, rg.x) : rg.x;
    id_nxt = list[min(cs + (uint32_t)lane, rg.x + maxn - 1u)];
  };
  auto load_rec = [&]() {
    id_cur = id_nxt;
    const float4* p = reinterpret_cast<const float4*>(splat + id_nxt);
    r0 = p[0]; r1 = p[1]; r2 = p[2];
  };
  auto consume = [&](uint32_t ce) {
    keep = false;
    const uint32_t cs = bwd_round_start(ce, rg.x);
    if ((uint32_t)lane < ce - cs) {
      keep = CULL ? (record_box_hits(r0.x, r0.y, r2.z, r2.w, wx0, wx1, wy0, wy1) &&
                     record_reaches_block(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r2.z, wx0, wx1, wy0, wy1)) : true;
      if (!CULL) r1.y = -__builtin_huge_valf();
      r2.z = r1.w;                                                   // r joins g, b
      r1.w = __uint_as_float((cs - rg.x) + (uint32_t)lane);          // 0-based list position
      r2.w = __uint_as_float((uint32_t)lane);                        // index inside the round
    }
  };

  uint32_t cend = rg.x + maxn;  // one past the last position that matters
  load_id(cend);
  load_rec();
  load_id(bwd_round_start(cend, rg.x));
  int par = 0;
  while (cend > rg.x) {
    const uint32_t cstart = bwd_round_start(cend, rg.x);
    const int n = (int)(cend - cstart);
    consume(cend);                                       // the records requested one round ago
    const uint64_t kept = __ballot(keep);
    const int nk = __popcll(kept), n8 = (nk + 7) & ~7;
    if (keep) {  // compacted, order preserved
      const int slot = __popcll(kept & lt_mask);
      rec[slot * 3 + 0] = r0; rec[slot * 3 + 1] = r1; rec[slot * 3 + 2] = r2;
    }
    bwd_stage_padding(rec, lane, nk, n8);
    if (wv == 0 && lane < n) { s_id[par][lane] = id_cur; s_cop[par][lane] = make_float4(r0.z, r0.w, r1.x, r1.z); }
    load_rec();                                          // next round's records
    load_id(cstart > rg.x ? bwd_round_start(cstart, rg.x) : rg.x); // and the list entries of the round after it
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    uint64_t touched = 0ull;
    for (int j0 = n8 - 8; j0 >= 0; j0 -= 8) {
      const float4* grp = rec + j0 * 3;
#pragma unroll
      for (int jj = 7; jj >= 0; --jj) {
        const float4 a = grp[jj * 3 + 0], b = grp[jj * 3 + 1];
        const float dy = a.y - pyf;
        const float nBdy = a.w * dy, hCdy2 = (b.x * dy) * dy;
        const uint32_t pos0 = __float_as_uint(b.w);
        const float dx = a.x - pxf;
        const float pw = __builtin_fmaf(__builtin_fmaf(a.z, dx, nBdy), dx, hCdy2);
        const uint64_t need = __ballot(pos0 < lastn) & __ballot(pw >= b.y);   // two compares into SGPR pairs + s_and
        if (need == 0ull) continue;
        const float4 c = grp[jj * 3 + 2];                            // g, b, r, index inside the round
        const float col[3] = {c.z, c.x, c.y};
        float s[8], sop;                                             // colour r g b | conic A B C | mean sums x y ; opacity
        const uint64_t live = bwd_update<EXP_MODE>(st, pw, dx, dy, need, b.z, col, s, sop);
        if (live != 0ull) {   // wave-uniform: somebody in this wave saw the Gaussian
          const uint32_t ridx = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(c.w));
          touched |= 1ull << ridx;
          const float tot = wave_reduce_swap<false>(s, sop, 0.0f);
          if (is_writer) s_sum[par][wv][ridx][writer_comp] = tot;
        }
      }
    }
    if (lane == 0) { s_touch[par][wv][0] = (uint32_t)touched; s_touch[par][wv][1] = (uint32_t)(touched >> 32); }
    __syncthreads();
    {
      // flush: the round's (record, component) sums over the workgroup's threads, component fastest -- s_sum keeps the
      // accumulator record's order (conic A B C | opacity | mean x y | colour r g b), so consecutive lanes add to
      // consecutive floats of one 48-byte record and the atomics of a record reach L2 as one or two requests
      // instead of nine (a lane per record and one component per instruction was bound by the L2 atomic units).
      // All waves' sums are combined and the per-record constants applied here (bwd_scale).
      uint64_t tw[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) tw[w] = (uint64_t)s_touch[par][w][0] | ((uint64_t)s_touch[par][w][1] << 32);
      for (int t = threadIdx.x; t < 64 * 9; t += 64 * NW) {
        const int r = t / 9, slot = t - 9 * r;
        if (r >= n) break;
        float v = 0.0f, swx = 0.0f, swy = 0.0f;
        bool hany = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const bool h = (tw[w] >> r) & 1ull;
          hany = hany || h;
          v += h ? s_sum[par][w][r][slot] : 0.0f;
          swx += h ? s_sum[par][w][r][GGD_ACC_MEAN2D] : 0.0f;
          swy += h ? s_sum[par][w][r][GGD_ACC_MEAN2D + 1] : 0.0f;
        }
        if (!hany) continue;
        const float4 co = s_cop[par][r];
        atomicAdd(grad_acc + GGD_ACC_FLOATS * (size_t)s_id[par][r] + slot,
                  bwd_scale(slot, v, swx, swy, co.x, co.y, co.z, co.w, ddelx_dx, ddely_dy));
      }
    }
    cend = cstart;
    par ^= 1;
  }
}


// ---- backward blend, quarter form: every 8x8 quarter of a tile is an INDEPENDENT single-wave workgroup --------------------
// No workgroup barrier and no cross-wave combine: a wave walks the tile's list back to front from ITS OWN last contributor,
// parks the per-record sums of a round in LDS in processing order (row = 9 sums + the record's slot in the staging area,
// where its id, opacity and conic still are), and flushes them itself -- (record, component) pairs over the lanes, component
// fastest, so a record's nine atomics form one 36-byte span -- at the top of the NEXT round, before that round's records
// overwrite the staging area and before its prefetch loads are issued: a wait for the loads then never waits for younger
// atomics (loads and atomics share one in-order counter).  Compared with the tile form a Gaussian that touches k quarters of
// a tile costs k coalesced atomic spans instead of one; in exchange the four quarters never wait for each other (the tile
// form spent 13 % / 28 % of its time in the per-round lock step: cube / shell), and the four quarters of a tile are placed in
// consecutive dispatch slots of one XCD like the forward's.
// STATS (ggd_blend_stats, debug): per-wave work counters added to stats[GGD_STATS_BWD ..] at the wave's end -- list entries the
// wave walks (its share of the tile's list up to its last contributor), records staged after the pre-cull, staged records some
// pixel still needed (`need`), records at least one pixel actually blended (`live`: a 9-sum reduction + a parked row each),
// the live lanes of those, rows flushed (= 36-byte atomic spans), gather rounds.
// AUX (ggd_backward_aux): the Gaussians' depths are staged in s_z next to their records; the depth is a fourth colour channel
// (background 0) whose per-record sum alpha T dL/ddepth is the TENTH reduced value and goes to slot 9 of the accumulator
// record (a pad word: layout and memset unchanged); dL/dalpha of a pixel only enters through its final transmittance, i.e. as
// -dL/dalpha folded into bgdot once.  Rows of 10 sums + slot and the staged depths: 6144 B of LDS per wave.  depth_keys,
// dL_ddepth and dL_dalpha are NULL, and never read, in a plain backward.
// ABS (ggd_backward_abs, with or without AUX): the per-pixel absolute values of the two mean-gradient components (bwd_update)
// are the ELEVENTH and TWELFTH reduced values (lanes 6 and 38), parked in two more columns of the row and added, times
// op * 0.5 W / op * 0.5 H, to slots GGD_ACC_ABS, GGD_ACC_ABS + 1 of the accumulator record (the two remaining pad words).
// Rows of 11 (AUX: 12) sums + slot: 6144 B of LDS per wave (AUX: 6656).  The ABS instances are kernels of their own,
// blend_backward_quarter_abs_kernel<EXP_MODE, CULL, AUX>, from the same text (ggd_blend_bwd_quarter.inc, included twice):
// blend_backward_quarter_kernel keeps its name, its four template arguments and its code.
#define GGD_BWDQ_TEMPLATE template <int EXP_MODE, bool CULL, bool STATS = false, bool AUX = false>
#define GGD_BWDQ_NAME blend_backward_quarter_kernel
#define GGD_BWDQ_LOCALS constexpr bool ABS = false;
#include "ggd_blend_bwd_quarter.inc"
#undef GGD_BWDQ_TEMPLATE
#undef GGD_BWDQ_NAME
#undef GGD_BWDQ_LOCALS
// the absgrad backward (no statistics instance: stats is NULL)
#define GGD_BWDQ_TEMPLATE template <int EXP_MODE, bool CULL, bool AUX = false>
#define GGD_BWDQ_NAME blend_backward_quarter_abs_kernel
#define GGD_BWDQ_LOCALS constexpr bool ABS = true, STATS = false;
#include "ggd_blend_bwd_quarter.inc"
#undef GGD_BWDQ_TEMPLATE
#undef GGD_BWDQ_NAME
#undef GGD_BWDQ_LOCALS

}  // namespace

int ggd_launch_blend(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                     const uint32_t* list, const uint32_t* ranges, uint32_t capacity, float* out_color, float* final_T,
                     uint32_t* n_contrib, const uint32_t* depth_keys, float* out_depth, float* out_alpha) {
  const int gx = (prm.width + 15) / 16, gy = (prm.height + 15) / 16;
  if (gx * gy == 0) return GGD_OK;
  const int em = ctx->opt[GGD_OPT_EXP_MODE] == 3 ? 1 : ctx->opt[GGD_OPT_EXP_MODE];   // 3 (default): bare v_exp_f32 in the forward
  const bool cull = ctx->opt[GGD_OPT_BLEND_CULL] != 0;
  const int T = gx * gy;
  static const int lds_pad = getenv("GGD_BLEND_LDS_PAD") ? atoi(getenv("GGD_BLEND_LDS_PAD")) : 0;   // experiment: caps the waves per CU
  const bool aux = out_depth || out_alpha;   // the depth / alpha extension
  if (aux && (!out_depth || !out_alpha || !depth_keys)) return ggd_fail(ctx, GGD_E_INVALID, "internal: depth / alpha blend needs both planes and the depth keys");
  // one instance per (exp mode, cull, variant); the variants exclude each other: an aux frame has no statistics instance
  // (ggd_blend_stats counts plain frames only)
  enum { PLAIN = 0, STATS = 1, AUX = 2 };
  const int variant = aux ? AUX : (ctx->blend_stats ? STATS : PLAIN);
  ggd_dispatch<3>(em, [&](auto e) {
    ggd_dispatch<2>(cull, [&](auto c) {
      ggd_dispatch<3>(variant, [&](auto v) {
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((blend_forward_kernel<decltype(e)::value, decltype(c)::value != 0, V == STATS, V == AUX>),
                           dim3(4 * T), dim3(64), lds_pad, s, prm.width, prm.height, gx, T, splat, list, ranges, capacity, prm.bg,
                           out_color, final_T, n_contrib, V == STATS ? ctx->blend_stats : nullptr,
                           V == AUX ? depth_keys : nullptr, out_depth, out_alpha);
      });
    });
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

int ggd_launch_blend_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_splat* splat,
                              const uint32_t* list, const uint32_t* ranges, const float* final_T,
                              const uint32_t* n_contrib, const ggd_pix_grads& pix, float* grad_acc, bool aux,
                              const uint32_t* depth_keys, bool abs) {
  const int gx = (prm.width + 15) / 16, gy = (prm.height + 15) / 16;
  if (gx * gy == 0) return GGD_OK;
  const int em = ctx->opt[GGD_OPT_EXP_MODE];   // 3 (default): compensated 2^x, contribution decision on the forward's bare v_exp_f32 value
  const bool cull = ctx->opt[GGD_OPT_BLEND_CULL] != 0;
  const int T = gx * gy;
  int split = ctx->opt[GGD_OPT_BLEND_SPLIT];
  // 4: four INDEPENDENT 8x8 quarter waves per tile (blend_backward_quarter_kernel); any other explicit value: the four
  // quarter waves of a tile in one workgroup, per-record sums combined in LDS (blend_backward_tile_kernel).  1 (auto): the
  // quarter form.  Until round 6 the rule sent grids below 2048 tiles to the tile form (round 3: 500 k / 512^2 184 vs 206 us);
  // with the quarter kernel's later changes (whole-record LDS prefetch, live-rectangle pre-cull, flush before the loads) it
  // is equal or faster on every grid measured -- 100 k / 512^2 54.9 vs 58.5 us, 30 k / 512^2 23.6 vs 24.9, 100 k / 256^2 55 vs 65,
  // 500 k / 512^2 cube 175 vs 173 (a tie), head-like 500 k / 512^2 (the train step's scenes) 281 vs 394 and 311 vs 484,
  // 1 M / 704^2 225 vs 250 (profiles/r06/backward_blend_form_ab.txt)
  if (split == 1) split = 4;
  static const int lds_pad = getenv("GGD_BLEND_BWD_LDS_PAD") ? atoi(getenv("GGD_BLEND_BWD_LDS_PAD")) : 0;   // experiment
  // the depth / alpha backward exists in the quarter form only: it is used whatever GGD_OPT_BLEND_SPLIT says (the tile form
  // is an explicit, non-default choice kept for measurements); so does the absgrad backward
  if (aux && !depth_keys) return ggd_fail(ctx, GGD_E_INVALID, "internal: depth / alpha backward needs the depth keys");
  if (!aux && !abs && split != 4) {
    ggd_dispatch<4>(em, [&](auto e) {
      ggd_dispatch<2>(cull, [&](auto c) {
        hipLaunchKernelGGL((blend_backward_tile_kernel<decltype(e)::value, decltype(c)::value != 0>), dim3(T), dim3(256), 0, s,
                           prm.width, prm.height, gx, gy, splat, list, ranges, prm.bg, final_T, n_contrib, pix.dL_dpix, grad_acc);
      });
    });
    GGD_HIP(hipGetLastError());
    return GGD_OK;
  }
  // quarter form, one instance per (exp mode, cull, variant); the variants exclude each other: no statistics instance of the
  // depth / alpha backward, nor of the absgrad ones (ABS, AUXABS: the absolute sums without / with the depth / alpha terms)
  enum { PLAIN = 0, STATS = 1, AUX = 2, ABS = 3, AUXABS = 4 };
  const int variant = abs ? (aux ? AUXABS : ABS) : (aux ? AUX : (ctx->blend_stats ? STATS : PLAIN));
  ggd_dispatch<4>(em, [&](auto e) {
    ggd_dispatch<2>(cull, [&](auto c) {
      ggd_dispatch<5>(variant, [&](auto v) {
        constexpr int V = decltype(v)::value, E = decltype(e)::value;
        constexpr bool C = decltype(c)::value != 0, VAUX = V == AUX || V == AUXABS;
        const auto kernel = (V == ABS || V == AUXABS) ? blend_backward_quarter_abs_kernel<E, C, VAUX>
                                                      : blend_backward_quarter_kernel<E, C, V == STATS, VAUX>;
        hipLaunchKernelGGL(kernel, dim3(4 * T), dim3(64), lds_pad, s, prm.width, prm.height, gx, gy, splat, list, ranges, prm.bg,
                           final_T, n_contrib, pix.dL_dpix, grad_acc, V == STATS ? ctx->blend_stats : nullptr,
                           VAUX ? depth_keys : nullptr, VAUX ? pix.dL_ddepth : nullptr, VAUX ? pix.dL_dalpha : nullptr);
      });
    });
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
