// ggd_rowbin_wide.inc -- the two-level row / column binning of ggd_rowbin.hip for tile grids beyond 64 x 64 (up to 255 x 255
// tiles: 4080 x 4080 pixels), included inside that file's anonymous namespace.
//
// Same algorithm, same six launches, same results (the lists and ranges of the radix-sort path, bit for bit); what changes
// is that a bin (tile row at level 1, tile column at level 2) is no longer a LANE but a (group, lane) pair, group = bin / 64:
// every per-bin quantity becomes a small register array over the groups, every prefix over the bins carries from one
// group into the next, and the emission transposes one 64 x 64 bit matrix per group an item round touches.  Until this
// path existed a 1080p frame took the single-level tile binning (550 us for 11 M instances) and anything above 8192 tiles
// the 64-bit radix sort (5.6 ms for the 75 M instances of a 4K frame).
// (RBW_NG = 4 groups of 64 bins, RBW_BINS = 256 and the tables RBW_TAB_*: ggd_binning_layout.h)

// inclusive prefix of an int over the 256 threads of the block (thread = bin); lds4: 4 ints
__device__ __forceinline__ int block_incl_scan_256_i32(int v, int* lds4) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inc = wave_inclusive_scan(v);
  if (lane == 63) lds4[wv] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) if (w < wv) base += lds4[w];
  return base + inc;
}

// ---- level 1 count (as rb_count1_kernel; counts1[block][nb], nb = 64 * groups of rows)
__global__ __launch_bounds__(RB_THREADS) void rbw_count1_kernel(const uint2* __restrict__ rect, const uint32_t* __restrict__ order,
                                                                const uint32_t* __restrict__ n_vis_ptr, int P, int nb,
                                                                uint2* __restrict__ packed, uint32_t* __restrict__ counts1,
                                                                const uint32_t* __restrict__ order_alt,
                                                                const uint32_t* __restrict__ use_alt) {
  __shared__ int diff[RBW_BINS + 1];
  __shared__ int carry[4];
  if (use_alt && *use_alt != 0u) order = order_alt;
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint32_t base = (uint32_t)blockIdx.x * RB_CHUNK;
  if (base >= n_vis) return;
  const int tid = threadIdx.x;
  diff[tid] = 0;
  if (tid == 0) diff[RBW_BINS] = 0;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const uint32_t rnk = base + (uint32_t)q * RB_THREADS + tid;
    if (rnk < n_vis) {
      const uint32_t id = order[rnk];
      const uint2 rc = rect[id];   // {minx | maxx << 16, miny | maxy << 16}, all <= 255 on the grids this path takes
      const int x0 = (int)(rc.x & 0xffffu), x1 = (int)(rc.x >> 16), y0 = (int)(rc.y & 0xffffu), y1 = (int)(rc.y >> 16);
      const int n = (x1 - x0) * (y1 - y0);
      packed[rnk] = make_uint2(id, n > 0 ? rb_pack_rect((uint32_t)x0, (uint32_t)x1, (uint32_t)y0, (uint32_t)y1) : 0u);
      if (n > 0) { atomicAdd(&diff[y0], 1); atomicAdd(&diff[y1], -1); }
    }
  }
  __syncthreads();
  const int inc = block_incl_scan_256_i32(diff[tid], carry);
  if (tid < nb) counts1[(size_t)blockIdx.x * nb + tid] = (uint32_t)inc;
}

// ---- level 1 scan, one workgroup: per row the exclusive prefix over the chunks, row starts, level-2 blocks per row
__global__ __launch_bounds__(1024) void rbw_scan1_kernel(uint32_t* __restrict__ counts1, const uint32_t* __restrict__ n_vis_ptr,
                                                         int P, int ng, uint32_t* __restrict__ tab, uint32_t ent_cap) {
  __shared__ uint32_t part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nbins = 64 * ng;
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint32_t nblk = (n_vis + RB_CHUNK - 1) / RB_CHUNK;
  uint32_t row_carry = 0, blk_carry = 0;   // wave 0: entries / level-2 blocks of the earlier groups
  for (int g = 0; g < ng; ++g) {
    const int bin = 64 * g + lane;
    const uint32_t tot = rb_prefix_over_chunks<8>(counts1, 0u, nblk, nbins, bin, part);
    if (wv == 0) {
      const uint32_t inc = row_carry + wave_inclusive_scan(tot);
      const uint32_t rs = inc - tot;
      tab[RBW_TAB_ROWSTART + bin] = rs;
      const uint32_t have = rs < ent_cap ? min(tot, ent_cap - rs) : 0u;   // see rb_write_row_tables
      const uint32_t nb2 = (have + RB_CHUNK - 1) / RB_CHUNK;
      const uint32_t binc = blk_carry + wave_inclusive_scan(nb2);
      tab[RBW_TAB_ROWBLK + bin] = binc - nb2;
      tab[RBW_TAB_FLAG + bin] = 0u;
      row_carry = wave_pick(inc, 63);
      blk_carry = wave_pick(binc, 63);
    }
    __syncthreads();   // part is reused by the next group
  }
  if (wv == 0) {
    // the table entries behind the last group (read by the block -> row search and by `row + 1`) hold the totals
    for (int b = nbins + lane; b <= RBW_BINS; b += 64) { tab[RBW_TAB_ROWSTART + b] = row_carry; tab[RBW_TAB_ROWBLK + b] = blk_carry; }
  }
}

// wave_cols / wave_emit of ggd_rowbin.hip with (group, lane) bins (round 5: counts from the transposes, item-parallel emission):
// cols[q][g] of lane l = the items of round q that cover bin 64 g + l (one transpose per group the round touches);
// cnt[g] = the wave's entries in bin 64 g + lane.
__device__ __forceinline__ void wave_cols_w(const uint32_t (&iv)[RB_IPL], int n_items, int ng, uint64_t (&cols)[RB_IPL][RBW_NG],
                                            uint32_t (&cnt)[RBW_NG]) {
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) cnt[g] = 0;
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const int l = (int)(iv[q] & 0xffu), h = (int)(iv[q] >> 8);
#pragma unroll
    for (int g = 0; g < RBW_NG; ++g) {
      cols[q][g] = 0ull;
      if (g >= ng || q * 64 >= n_items) continue;
      const int lg = min(max(l - 64 * g, 0), 64), hg = min(max(h - 64 * g, 0), 64);
      const uint64_t below_h = hg >= 64 ? ~0ull : ((1ull << hg) - 1ull);
      const uint64_t below_l = lg >= 64 ? ~0ull : ((1ull << lg) - 1ull);
      const uint64_t row = (h > l && hg > lg) ? (below_h & ~below_l) : 0ull;
      if (__ballot(row != 0ull) == 0ull) continue;   // nobody in this round touches the group
      cols[q][g] = wave_transpose64(row);
      cnt[g] += (uint32_t)__popcll(cols[q][g]);
    }
  }
}

// item-parallel emission: the lane keeps its item and walks the bins it covers; per bin one {mask, destination} look-up in the
// wave's LDS slab (256 bins: s_col 2 KB + s_dst 1 KB per wave).  dst[g] = this lane's running destination in bin 64 g + lane.
template <bool TWO, typename Emit>
__device__ __forceinline__ void wave_emit_w(const uint32_t (&iv)[RB_IPL], const uint32_t (&pa)[RB_IPL],
                                            const uint32_t (&pb)[RB_IPL], const uint64_t (&cols)[RB_IPL][RBW_NG], int n_items, int ng,
                                            uint32_t (&dst)[RBW_NG], uint2* s_col /* [256], this wave's */, uint32_t* s_dst,
                                            Emit&& emit) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    if (q * 64 >= n_items) continue;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int g = 0; g < RBW_NG; ++g) {
      if (g >= ng) continue;
      s_col[64 * g + lane] = make_uint2((uint32_t)cols[q][g], (uint32_t)(cols[q][g] >> 32));
      s_dst[64 * g + lane] = dst[g];
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t l = iv[q] & 0xffu, h = iv[q] >> 8;
    uint32_t fill = 0;
#pragma unroll
    for (int g = 0; g < RBW_NG; ++g) fill = max(fill, (uint32_t)__popcll(cols[q][g]));
    if (rb_walk_items(h > l ? h - l : 0u, fill)) {
      for (uint32_t b = l; __ballot(b < h) != 0ull; ++b) {
        const bool act = b < h;
        const uint2 c = s_col[act ? b : 0u];
        const uint32_t d = s_dst[act ? b : 0u];
        const uint64_t m = (uint64_t)c.x | ((uint64_t)c.y << 32);
        if (act) emit(d + (uint32_t)__popcll(m & lt_mask), pa[q], TWO ? pb[q] : 0u);
      }
#pragma unroll
      for (int g = 0; g < RBW_NG; ++g) dst[g] += (uint32_t)__popcll(cols[q][g]);
    } else {   // bin-parallel drain, group by group (see wave_emit)
#pragma unroll
      for (int g = 0; g < RBW_NG; ++g) {
        uint64_t col = cols[q][g];
        while (__ballot(col != 0ull) != 0ull) {
          const bool act = col != 0ull;
          const int k = act ? (__ffsll((unsigned long long)col) - 1) : 0;
          col &= col - 1ull;
          const uint32_t a = (uint32_t)__shfl((int)pa[q], k, 64);
          const uint32_t bb = TWO ? (uint32_t)__shfl((int)pb[q], k, 64) : 0u;
          if (act) { emit(dst[g], a, bb); dst[g] += 1; }
        }
      }
    }
  }
}

// ---- level 1 scatter: {id, x0 | x1 << 8} into the list of every row in [y0, y1)
__global__ __launch_bounds__(RB_THREADS) void rbw_scatter1_kernel(const uint2* __restrict__ packed,
                                                                  const uint32_t* __restrict__ n_vis_ptr, int P, int ng,
                                                                  const uint32_t* __restrict__ prefix1,
                                                                  const uint32_t* __restrict__ tab,
                                                                  uint2* __restrict__ ent, uint32_t ent_cap) {
  __shared__ uint2 s_col[RB_WAVES][RBW_BINS];
  __shared__ uint32_t s_dst[RB_WAVES][RBW_BINS];
  __shared__ uint32_t wcnt[RB_WAVES][RBW_BINS];
  const uint32_t n_vis = min((uint32_t)P, *n_vis_ptr);
  const uint32_t base = (uint32_t)blockIdx.x * RB_CHUNK;
  if (base >= n_vis) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbins = 64 * ng;
  const uint32_t wbeg = base + (uint32_t)wv * RB_WCHUNK;
  const int n_items = (int)min((uint32_t)RB_WCHUNK, n_vis > wbeg ? n_vis - wbeg : 0u);
  uint32_t iv[RB_IPL], pa[RB_IPL], pb[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const int i = q * 64 + lane;
    uint2 it = make_uint2(0, 0);
    if (i < n_items) it = packed[wbeg + i];
    pa[q] = it.x; pb[q] = rb_packed_cols(it.y);
    iv[q] = rb_packed_rows(it.y);
  }
  uint32_t mine[RBW_NG];
  uint64_t cols[RB_IPL][RBW_NG];
  wave_cols_w(iv, n_items, ng, cols, mine);
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) if (g < ng) wcnt[wv][64 * g + lane] = mine[g];
  __syncthreads();
  uint32_t dst[RBW_NG];
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) {
    dst[g] = 0;
    if (g < ng) {
      const int bin = 64 * g + lane;
      uint32_t d = tab[RBW_TAB_ROWSTART + bin] + prefix1[(size_t)blockIdx.x * nbins + bin];
#pragma unroll
      for (int w = 0; w < RB_WAVES; ++w) if (w < wv) d += wcnt[w][bin];
      dst[g] = d;
    }
  }
  wave_emit_w<true>(iv, pa, pb, cols, n_items, ng, dst, s_col[wv], s_dst[wv], [&](uint32_t d, uint32_t id, uint32_t xx) {
    if (d < ent_cap) ent[d] = make_uint2(id, xx);
  });
}

// level-2 block -> (row, chunk within the row): the last row whose first block is <= blk (rows without blocks share the
// first block of the next row that has some, and lose to it)
__device__ __forceinline__ bool rbw_block_row(const uint32_t* __restrict__ tab, uint32_t blk, int& row, uint32_t& chunk) {
  const int lane = threadIdx.x & 63;
  const uint32_t total = tab[RBW_TAB_ROWBLK + RBW_BINS];
  if (blk >= total) return false;
  int r = -1;
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) r += __popcll(__ballot(tab[RBW_TAB_ROWBLK + 64 * g + lane] <= blk));
  row = r; chunk = blk - tab[RBW_TAB_ROWBLK + r];
  return true;
}

__global__ __launch_bounds__(RB_THREADS) void rbw_count2_kernel(const uint2* __restrict__ ent, uint32_t ent_cap,
                                                                const uint32_t* __restrict__ tab, int nb,
                                                                uint32_t* __restrict__ counts2) {
  __shared__ int diff[RBW_BINS + 1];
  __shared__ int carry[4];
  int row; uint32_t chunk;
  if (!rbw_block_row(tab, blockIdx.x, row, chunk)) return;
  const int tid = threadIdx.x;
  diff[tid] = 0;
  if (tid == 0) diff[RBW_BINS] = 0;
  __syncthreads();
  const uint32_t rbeg = tab[RBW_TAB_ROWSTART + row], rend = min(tab[RBW_TAB_ROWSTART + row + 1], ent_cap);
  const uint32_t base = rbeg + chunk * RB_CHUNK;
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const uint32_t i = base + (uint32_t)q * RB_THREADS + tid;
    if (i < rend) {
      const uint32_t xx = ent[i].y;
      const uint32_t x0 = xx & 0xffu, x1 = (xx >> 8) & 0xffu;
      if (x1 > x0) { atomicAdd(&diff[x0], 1); atomicAdd(&diff[x1], -1); }
    }
  }
  __syncthreads();
  const int inc = block_incl_scan_256_i32(diff[tid], carry);
  if (tid < nb) counts2[(size_t)blockIdx.x * nb + tid] = (uint32_t)inc;
}

// ---- level-2 scan, one workgroup per tile row (as rb_scan2_kernel): prefix over the row's chunks per column, tile totals,
//      tile starts; the rows below are summed from their published totals
__global__ __launch_bounds__(1024) void rbw_scan2_kernel(uint32_t* __restrict__ counts2, uint32_t* tab, int gx, int gy, int ng,
                                                         uint32_t* __restrict__ ranges) {
  __shared__ uint32_t part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nbins = 64 * ng;
  const int r = blockIdx.x;
  const uint32_t b0 = tab[RBW_TAB_ROWBLK + r], b1 = tab[RBW_TAB_ROWBLK + r + 1];
  uint32_t tots[RBW_NG];
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) {
    tots[g] = 0;
    if (g >= ng) continue;
    tots[g] = rb_prefix_over_chunks<4>(counts2, b0, b1 - b0, nbins, 64 * g + lane, part);
    __syncthreads();   // part is reused by the next group
  }
  if (wv == 0) {
    uint32_t incs[RBW_NG];
    uint32_t carry = 0;
#pragma unroll
    for (int g = 0; g < RBW_NG; ++g) {
      incs[g] = carry + wave_inclusive_scan(tots[g]);
      carry = wave_pick(incs[g], 63);
    }
    const uint32_t rowbase = rb_publish_row_sum_above(tab + RBW_TAB_ROWINST, tab + RBW_TAB_FLAG, r, carry);   // carry = instances of this row
#pragma unroll
    for (int g = 0; g < RBW_NG; ++g) {
      const int col = 64 * g + lane;
      if (g < ng) {
        const uint32_t start = rowbase + incs[g] - tots[g];
        tab[RBW_TAB_TILESTART + r * RBW_BINS + col] = start;
        if (col < gx) {
          const int t = r * gx + col;
          ranges[2 * t] = tots[g] ? start : 0u;
          ranges[2 * t + 1] = tots[g] ? start + tots[g] : 0u;
        }
      }
    }
  }
}

__global__ __launch_bounds__(RB_THREADS) void rbw_scatter2_kernel(const uint2* __restrict__ ent, uint32_t ent_cap,
                                                                  const uint32_t* __restrict__ tab, int ng,
                                                                  const uint32_t* __restrict__ prefix2,
                                                                  uint32_t* __restrict__ list, uint32_t capacity,
                                                                  uint32_t main_blocks, ggd_scan_piggy pg) {
  __shared__ uint2 s_col[RB_WAVES][RBW_BINS];
  __shared__ uint32_t s_dst[RB_WAVES][RBW_BINS];
  __shared__ uint32_t wcnt[RB_WAVES][RBW_BINS];
  __shared__ uint32_t stage[RB_STAGE];
  __shared__ uint32_t s_n[RBW_BINS], s_b0[RBW_BINS], s_g[RBW_BINS];   // per column: instances, LDS base, list destination
  if (blockIdx.x >= main_blocks) {   // appended workgroups: last step of the offsets scan (see ggd_scan_piggy)
    scan_apply_block(pg.in, pg.out, pg.n, pg.block_sums, (int)(blockIdx.x - main_blocks), stage, pg.sum_stride);
    return;
  }
  int row; uint32_t chunk;
  if (!rbw_block_row(tab, blockIdx.x, row, chunk)) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nbins = 64 * ng;
  const uint32_t rbeg = tab[RBW_TAB_ROWSTART + row], rend = min(tab[RBW_TAB_ROWSTART + row + 1], ent_cap);
  const uint32_t wbeg = rbeg + chunk * RB_CHUNK + (uint32_t)wv * RB_WCHUNK;
  const int n_items = (int)min((uint32_t)RB_WCHUNK, rend > wbeg ? rend - wbeg : 0u);
  uint32_t iv[RB_IPL], pa[RB_IPL], pb[RB_IPL];
#pragma unroll
  for (int q = 0; q < RB_IPL; ++q) {
    const int i = q * 64 + lane;
    uint2 it = make_uint2(0, 0);
    if (i < n_items) it = ent[wbeg + i];
    pa[q] = it.x; pb[q] = 0;
    iv[q] = it.y & 0xffffu;   // x0 | x1 << 8
  }
  uint32_t mine[RBW_NG];
  uint64_t cols[RB_IPL][RBW_NG];
  wave_cols_w(iv, n_items, ng, cols, mine);
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) if (g < ng) wcnt[wv][64 * g + lane] = mine[g];
  __syncthreads();
  uint32_t gbase[RBW_NG], before[RBW_NG], coltot[RBW_NG], colbeg[RBW_NG];
  uint32_t carry = 0;
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) {
    gbase[g] = before[g] = coltot[g] = colbeg[g] = 0;
    if (g < ng) {
      const int col = 64 * g + lane;
      gbase[g] = tab[RBW_TAB_TILESTART + row * RBW_BINS + col] + prefix2[(size_t)blockIdx.x * nbins + col];
#pragma unroll
      for (int w = 0; w < RB_WAVES; ++w) { const uint32_t c = wcnt[w][col]; if (w < wv) before[g] += c; coltot[g] += c; }
      const uint32_t colend = carry + wave_inclusive_scan(coltot[g]);   // same in every wave
      colbeg[g] = colend - coltot[g];
      carry = wave_pick(colend, 63);
    }
  }
  const uint32_t total = carry;
  if (total <= (uint32_t)RB_STAGE) {   // staged copy-out as rb_emit_chunk's, over (group, lane) bins: the runs' ends go through LDS
    uint32_t ldst[RBW_NG];
#pragma unroll
    for (int g = 0; g < RBW_NG; ++g) {
      ldst[g] = colbeg[g] + before[g];
      if (wv == 0 && g < ng) { s_n[64 * g + lane] = coltot[g]; s_b0[64 * g + lane] = colbeg[g]; s_g[64 * g + lane] = gbase[g]; }
    }
    wave_emit_w<false>(iv, pa, pb, cols, n_items, ng, ldst, s_col[wv], s_dst[wv], [&](uint32_t d, uint32_t id, uint32_t) { stage[d] = id; });
    __syncthreads();
    for (int c = wv; c < nbins; c += RB_WAVES) {
      const uint32_t n = s_n[c];
      if (n == 0) continue;
      const uint32_t b0 = s_b0[c], gd = s_g[c];
      for (uint32_t k = lane; k < n; k += 64) {
        const uint32_t d = gd + k;
        if (d < capacity) list[d] = stage[b0 + k];
      }
    }
    return;
  }
  uint32_t dst[RBW_NG];
#pragma unroll
  for (int g = 0; g < RBW_NG; ++g) dst[g] = gbase[g] + before[g];
  wave_emit_w<false>(iv, pa, pb, cols, n_items, ng, dst, s_col[wv], s_dst[wv], [&](uint32_t d, uint32_t id, uint32_t) {
    if (d < capacity) list[d] = id;
  });
}
