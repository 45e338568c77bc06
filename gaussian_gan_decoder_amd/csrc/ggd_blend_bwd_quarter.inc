// ggd_blend_bwd_quarter.inc -- the text of the quarter-form backward blend kernel (described in ggd_blend.hip, which includes
// this file once per kernel NAME: blend_backward_quarter_kernel and, with ABS on, blend_backward_quarter_abs_kernel).  Two
// kernels from one text, not one template with a fifth argument: the existing kernel keeps its name, its template arguments
// and, instruction for instruction, its code.  The including file defines
//   GGD_BWDQ_TEMPLATE   the template head (EXP_MODE, CULL, AUX; STATS where the kernel has a statistics instance)
//   GGD_BWDQ_NAME       the kernel's name
//   GGD_BWDQ_LOCALS     constexpr definitions of ABS and, where it is no template argument, STATS
GGD_BWDQ_TEMPLATE
__global__ __launch_bounds__(64) void GGD_BWDQ_NAME(
    int W, int H, int gx, int gy, const ggd_splat* __restrict__ splat, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ ranges, const float* __restrict__ bg, const float* __restrict__ final_T,
    const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dpix, float* __restrict__ grad_acc,
    unsigned long long* __restrict__ stats, const uint32_t* __restrict__ depth_keys, const float* __restrict__ dL_ddepth,
    const float* __restrict__ dL_dalpha) {
  GGD_BWDQ_LOCALS
  constexpr int NS = (AUX ? 10 : 9) + (ABS ? 2 : 0), ROW = NS + 1;   // reduced sums per record; parked row = sums | staging slot
  uint32_t st_staged = 0, st_need = 0, st_live = 0, st_lanes = 0, st_spans = 0, st_rounds = 0;
  __shared__ float4 s_rec[64 * 3];
  // [touched record, in processing order][NS sums | staging slot] (5632 B of LDS per wave with s_rec; AUX: 6144 with s_z); ONE
  // buffer: a round's rows are flushed at the top of the next round, before that round's first row is written (LDS operations
  // of a wave execute in order)
  __shared__ float s_sum[64][ROW];
  __shared__ float s_z[AUX ? 64 : 1];   // AUX: the staged records' depths (unused, and not allocated, otherwise)
  const int lane = threadIdx.x;
  int tile, sub;
  ggd_block_to_tile((int)blockIdx.x, 4, gx * gy, tile, sub);
  const int tx = tile % gx, ty = tile / gx;
  const int qx = sub & 1, qy = sub >> 1;
  const int px0 = tx * 16 + qx * 8 + (lane & 7), py = ty * 16 + qy * 8 + (lane >> 3);
  const uint2 rg = reinterpret_cast<const uint2*>(ranges)[tile];
  const bool in = py < H && px0 < W;
  const size_t HW = (size_t)H * W;
  const size_t pix0 = (size_t)py * W + px0;

  std::conditional_t<AUX, BwdPixelAux, BwdPixel> st;
  const float pxf = (float)px0, pyf = (float)py;
  const uint32_t lastn = bwd_pixel_init<AUX>(st, in, pix0, HW, bg, final_T, n_contrib, dL_dpix, dL_ddepth, dL_dalpha);
  uint32_t maxn = lastn;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) maxn = max(maxn, (uint32_t)__shfl_xor((int)maxn, d, 64));
  maxn = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxn);
  if (maxn == 0) return;
  const float ddelx_dx = 0.5f * (float)W, ddely_dy = 0.5f * (float)H;
  const float wx0 = (float)(tx * 16 + qx * 8), wy0 = (float)(ty * 16 + qy * 8);   // this wave's pixel rectangle
  const float wx1 = wx0 + 7.0f, wy1 = wy0 + 7.0f;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  // the writer lanes put their sum where it goes in the row (accumulator-record order); lane 2 adds the record's staging slot
  // to the same LDS store
  bool is_writer;
  const int writer_comp = bwd_writer_comp<AUX, ABS>(lane, is_writer);
  const bool stores = is_writer || lane == 2;
  const int store_col = is_writer ? writer_comp : NS;

  // staged = the record as loaded with three words replaced in place:
  //   {x, y, hA, nB} {hC, power threshold, opacity, 0-based list position} {g, b, r, Gaussian id}
  bool keep = false;
  uint32_t id_cur = 0, id_nxt = 0;
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0;    // x y hA nB | hC thr opacity r | g b ex ey
  uint32_t zk = 0;                                          // AUX: depth key of the record in r0..r2
  const uint32_t last_pos = rg.x + maxn - 1u;
  auto load_id = [&](uint32_t ce) {
    const uint32_t cs = ce > rg.x ? bwd_round_start(ce, rg.x) : rg.x;
    id_nxt = list[min(cs + (uint32_t)lane, last_pos)];
  };
  auto load_rec = [&]() {
    id_cur = id_nxt;
    const float4* p = reinterpret_cast<const float4*>(splat + id_nxt);
    r0 = p[0]; r1 = p[1]; r2 = p[2];
    if constexpr (AUX) zk = depth_keys[id_nxt];
  };
  // the pre-cull rectangle of a round = the bounding rectangle of the pixels that can see ANY record of the round (those
  // whose last contributor lies at or behind the round's first position): walking back to front a wave starts at its
  // deepest pixel, and until the others join, most records only reach pixels that are not live yet
  float lx0 = wx0, lx1 = wx1, ly0 = wy0, ly1 = wy1;
  auto shrink_rect = [&](uint32_t first_pos) {   // 0-based list position of the round's first record
    const uint64_t live = __ballot(lastn > first_pos);
    if (live != 0ull) {
      const int rmin = __builtin_ctzll(live) >> 3, rmax = (63 - __builtin_clzll(live)) >> 3;
      uint32_t m = (uint32_t)live | (uint32_t)(live >> 32);
      m |= m >> 16; m |= m >> 8; m &= 0xffu;
      const int cmin = __builtin_ctz(m), cmax = 31 - __builtin_clz(m);
      lx0 = wx0 + (float)cmin; lx1 = wx0 + (float)cmax;
      ly0 = wy0 + (float)rmin; ly1 = wy0 + (float)rmax;
    }
  };
  auto consume = [&](uint32_t ce) {
    keep = false;
    const uint32_t cs = bwd_round_start(ce, rg.x);
    if (CULL) shrink_rect(cs - rg.x);
    if ((uint32_t)lane < ce - cs) {
      keep = CULL ? (record_box_hits(r0.x, r0.y, r2.z, r2.w, lx0, lx1, ly0, ly1) &&
                     record_reaches_block(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r2.z, lx0, lx1, ly0, ly1)) : true;
      if (!CULL) r1.y = -__builtin_huge_valf();
      r2.z = r1.w;
      r1.w = __uint_as_float((cs - rg.x) + (uint32_t)lane);
      r2.w = __uint_as_float(id_cur);
    }
  };
  // the flush of one round's parked sums (cnt rows), reading the round's records where they were staged
  auto flush = [&](int cnt) {
    const float* rows = &s_sum[0][0];
    for (int p = lane; p < cnt * NS; p += 64) {
      const int r = p / NS, comp = p - NS * r;
      const float v = rows[r * ROW + comp];
      const float swx = rows[r * ROW + GGD_ACC_MEAN2D], swy = rows[r * ROW + GGD_ACC_MEAN2D + 1];
      const int slot = (int)__float_as_uint(rows[r * ROW + NS]);
      const float4 a = s_rec[slot * 3 + 0], b = s_rec[slot * 3 + 1];
      const uint32_t id = __float_as_uint(s_rec[slot * 3 + 2].w);
      if constexpr (ABS) {
        // the two absolute sums come last in the row: |conic map| was applied per pixel, the non-negative rest here
        const bool isabs = comp >= NS - 2;
        const float sc = b.z * (comp == NS - 2 ? ddelx_dx : ddely_dy);
        atomicAdd(grad_acc + GGD_ACC_FLOATS * (size_t)id + (isabs ? GGD_ACC_ABS + (comp - (NS - 2)) : comp),
                  isabs ? sc * v : bwd_scale(comp, v, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
      } else {
        atomicAdd(grad_acc + GGD_ACC_FLOATS * (size_t)id + comp,
                  bwd_scale(comp, v, swx, swy, a.z, a.w, b.x, b.z, ddelx_dx, ddely_dy));
      }
    }
  };

  uint32_t cend = rg.x + maxn;  // one past the last position this quarter needs
  load_id(cend);
  load_rec();
  load_id(bwd_round_start(cend, rg.x));
  int prev_cnt = 0;
  while (cend > rg.x) {
    const uint32_t cstart = bwd_round_start(cend, rg.x);
    consume(cend);                                       // the records requested one round ago
    __builtin_amdgcn_wave_barrier();                     // (the previous round's LDS reads are done: in-order per wave)
    flush(prev_cnt);                                     // the previous round's sums: BEFORE its records are overwritten and
    __builtin_amdgcn_wave_barrier();                     // before the new loads are issued
    const uint64_t kept = __ballot(keep);
    const int nk = __popcll(kept), n8 = (nk + 7) & ~7;
    if (STATS) { st_staged += (uint32_t)nk; st_rounds += 1; st_spans += (uint32_t)prev_cnt; }
    if (keep) {  // compacted, order preserved
      const int slot = __popcll(kept & lt_mask);
      s_rec[slot * 3 + 0] = r0; s_rec[slot * 3 + 1] = r1; s_rec[slot * 3 + 2] = r2;
      if constexpr (AUX) s_z[slot] = __uint_as_float(zk);   // view-space depth (the key is its fp32 bits)
    }
    bwd_stage_padding(s_rec, lane, nk, n8);
    load_rec();                                          // next round's records
    load_id(cstart > rg.x ? bwd_round_start(cstart, rg.x) : rg.x); // and the list entries of the round after it
    __builtin_amdgcn_wave_barrier();
    int cnt = 0;
    float* rows = &s_sum[0][0];
    for (int j0 = n8 - 8; j0 >= 0; j0 -= 8) {
      uint32_t ga = (uint32_t)(uintptr_t)(lds_cf4*)(s_rec + j0 * 3);   // see blend_forward_kernel
      asm volatile("" : "+v"(ga));
      lds_cf4* grp = (lds_cf4*)(uintptr_t)ga;
      // (all twelve words one record ahead, inside the group: see the forward)
      float4 a_nx = lds_read4(grp + 7 * 3), b_nx = lds_read4(grp + 7 * 3 + 1), c_nx = lds_read4(grp + 7 * 3 + 2);
      const float* zgrp = AUX ? s_z + j0 : nullptr;
      float z_nx = 0.0f;
      if constexpr (AUX) z_nx = zgrp[7];
#pragma unroll
      for (int jj = 7; jj >= 0; --jj) {
        const float4 a = a_nx, b = b_nx, c4 = c_nx;
        const float z = z_nx;
        asm volatile("" : : "v"(c4.w));   // (keeps the unused twelfth word's VGPR from being handed out while the load is in flight)
        if (jj > 0) {
          a_nx = lds_read4(grp + (jj - 1) * 3); b_nx = lds_read4(grp + (jj - 1) * 3 + 1); c_nx = lds_read4(grp + (jj - 1) * 3 + 2);
          if constexpr (AUX) z_nx = zgrp[jj - 1];
        }
        const float dy = a.y - pyf;
        const float nBdy = a.w * dy, hCdy2 = (b.x * dy) * dy;
        const uint32_t pos0 = __float_as_uint(b.w);
        const float dx = a.x - pxf;
        const float pw = __builtin_fmaf(__builtin_fmaf(a.z, dx, nBdy), dx, hCdy2);
        const uint64_t need = __ballot(pos0 < lastn) & __ballot(pw >= b.y);
        if (need == 0ull) continue;
        if (STATS) st_need += 1;
        const float col[3] = {c4.z, c4.x, c4.y};                     // r | g, b
        float s[8], sop, sz = 0.0f;                                  // colour r g b | conic A B C | mean sums x y ; opacity ; depth
        float sabs[2] = {0.0f, 0.0f};                                // ABS: |mean x|, |mean y| of this pixel
        const uint64_t live = bwd_update<EXP_MODE, AUX, ABS>(st, pw, dx, dy, need, b.z, col, s, sop, z, &sz, a.z, a.w, b.x, sabs);
        if (live != 0ull) {   // wave-uniform: somebody in this wave saw the Gaussian
          if (STATS) { st_live += 1; st_lanes += (uint32_t)__popcll(live); }
          const float tot = wave_reduce_swap<AUX, ABS>(s, sop, sz, sabs[0], sabs[1]);
          // the writer lanes' sums (bwd_writer_comp); lane 2 the record's slot in the staging area
          const float v = is_writer ? tot : __uint_as_float((uint32_t)(j0 + jj));
          if (stores) rows[cnt * ROW + store_col] = v;
          ++cnt;
        }
      }
    }
    prev_cnt = cnt;
    cend = cstart;
  }
  __builtin_amdgcn_wave_barrier();
  flush(prev_cnt);
  if (STATS && lane == 0 && stats) {
    unsigned long long* o = stats + GGD_STATS_BWD;
    atomicAdd(o + 0, (unsigned long long)maxn);
    atomicAdd(o + 1, (unsigned long long)st_staged);
    atomicAdd(o + 2, (unsigned long long)st_need);
    atomicAdd(o + 3, (unsigned long long)st_live);
    atomicAdd(o + 4, (unsigned long long)st_lanes);
    atomicAdd(o + 5, (unsigned long long)(st_spans + (uint32_t)prev_cnt));
    atomicAdd(o + 6, (unsigned long long)st_rounds);
    atomicAdd(o + 7, 1ull);
  }
}
