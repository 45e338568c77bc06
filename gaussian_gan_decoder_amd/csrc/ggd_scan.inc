// ggd_scan.inc -- workgroup-level pieces of the uint32 prefix scan (stage a5), included inside the anonymous namespace of
// the translation units that run them: ggd_binning.hip (the scan kernels; the depth sort's appended workgroups) and
// ggd_rowbin.hip (the apply step as appended workgroups of the last binning launch).  The wave scan under them is
// wave_inclusive_scan of ggd_lanes.h, which the including file includes first (outside its namespace).
// ------------------------------------------------------------------------------------------------ block scan --
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;                        // per thread
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;  // 2048 per block

// Exclusive prefix of `v` over the 256 threads of the block (4 waves); *total = block sum.
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* total, uint32_t* lds4) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t inc = wave_inclusive_scan(v);
  if (lane == 63) lds4[wv] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s = lds4[w];
    if (w < wv) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// The three steps of the scan as workgroup-level functions: launched as their own kernels (two-call forward, sort path) or
// run by EXTRA workgroups appended to the depth sort's first three launches (single-call forward: nothing on that path
// reads the offsets or the total before the frame ends, so the scan needs no launches of its own -- see ggd_scan_piggy).
__device__ __forceinline__ void scan_reduce_block(const uint32_t* __restrict__ in, int64_t n,
                                                  uint32_t* __restrict__ block_sums, int blk, uint32_t* lds4) {
  const int64_t base = (int64_t)blk * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t s = 0;
  if (base + SCAN_ITEMS <= n) {
    const uint4 a = *reinterpret_cast<const uint4*>(in + base);
    const uint4 b = *reinterpret_cast<const uint4*>(in + base + 4);
    s = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
  } else {
    for (int k = 0; k < SCAN_ITEMS; ++k)
      if (base + k < n) s += in[base + k];
  }
  uint32_t tot;
  block_exclusive_scan_256(s, &tot, lds4);
  if (threadIdx.x == 0) block_sums[blk] = tot;
}

// One workgroup turns block_sums[nb] into exclusive block prefixes (in place) and writes the grand total -- also straight
// into the pinned host mirror (h_total: no blit kernel for the num_rendered read-back).
__device__ __forceinline__ void scan_blocksums_block(uint32_t* __restrict__ block_sums, int nb,
                                                     uint32_t* __restrict__ d_total, uint32_t* h_total, uint32_t* lds4,
                                                     unsigned long long* h_tagged = nullptr, uint32_t tag = 0) {
  uint32_t carry = 0;
  for (int start = 0; start < nb; start += SCAN_THREADS) {
    const int i = start + threadIdx.x;
    const uint32_t v = i < nb ? block_sums[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan_256(v, &tot, lds4);
    if (i < nb) block_sums[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0 && d_total) *d_total = carry;
  if (threadIdx.x == 0 && h_total) { *h_total = carry; __threadfence_system(); }
  if (threadIdx.x == 0 && h_tagged) {   // one 64-bit store: the host sees tag and total together
    __hip_atomic_store(h_tagged, ((unsigned long long)tag << 32) | carry, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Step 2 of a scan whose step 1 was done by the preprocess kernel (ggd_fold): info[i] = {sum of tiles_touched, kept keys, ~(smallest
// kept key), largest kept key} of 256-point workgroup i ({.., 0, 0} when it kept nothing).  One workgroup writes the exclusive prefixes of the sums to block_prefix[n_info], the grand total
// (num_rendered) where scan_blocksums_block writes it, and the number of kept keys to *n_valid.  Four entries per thread and
// round: 1 M points = 3907 entries = 4 rounds.
// Returns {num_rendered, kept keys, ~min key, max key} in every thread (the frame's kept-key range: the two-launch sort's next
// windows are fitted to it); the tagged host word is left to the caller (it adds a flag).
__device__ __forceinline__ uint4 scan_info_block(const uint4* __restrict__ info, int n_info, uint32_t* __restrict__ block_prefix,
                                                 uint32_t* __restrict__ n_valid, uint32_t* __restrict__ d_total, uint32_t* h_total,
                                                 uint32_t* lds4) {
  uint32_t carry = 0, valid = 0, nmin = 0, kmax = 0;
  // (this workgroup rides on a launch whose other workgroups take ~8 us: as a chain of dependent rounds -- load, scan, store -- it
  // was the launch's critical path, 12.7 us at 1 M points; the records of up to four rounds are requested together)
  constexpr int ROUNDS = 4;
  for (int start0 = 0; start0 < n_info; start0 += ROUNDS * 4 * SCAN_THREADS) {
    uint4 e[ROUNDS][4];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = start0 + r * 4 * SCAN_THREADS + 4 * (int)threadIdx.x + k;
        e[r][k] = i < n_info ? info[i] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int i0 = start0 + r * 4 * SCAN_THREADS + 4 * (int)threadIdx.x;
      if (start0 + r * 4 * SCAN_THREADS >= n_info) break;     // (uniform)
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] = e[r][k].x; valid += e[r][k].y; nmin = max(nmin, e[r][k].z); kmax = max(kmax, e[r][k].w); }
      uint32_t tot;
      uint32_t run = carry + block_exclusive_scan_256(v[0] + v[1] + v[2] + v[3], &tot, lds4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i0 + k < n_info) block_prefix[i0 + k] = run;
        run += v[k];
      }
      carry += tot;
    }
  }
  uint32_t vtot;
  block_exclusive_scan_256(valid, &vtot, lds4);
  nmin = wave_max_lane63(nmin);
  kmax = wave_max_lane63(kmax);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) { lds4[threadIdx.x >> 6] = nmin; lds4[4 + (threadIdx.x >> 6)] = kmax; }   // (callers pass >= 8 words)
  __syncthreads();
  nmin = max(max(lds4[0], lds4[1]), max(lds4[2], lds4[3]));
  kmax = max(max(lds4[4], lds4[5]), max(lds4[6], lds4[7]));
  __syncthreads();
  if (threadIdx.x == 0 && n_valid) *n_valid = vtot;
  if (threadIdx.x == 0 && d_total) *d_total = carry;
  if (threadIdx.x == 0 && h_total) { *h_total = carry; __threadfence_system(); }
  return make_uint4(carry, vtot, nmin, kmax);
}

// pstride: block_prefix entries per 2048-element block (1; 8 when the prefixes are per 256-point preprocess workgroup)
__device__ __forceinline__ void scan_apply_block(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n,
                                                 const uint32_t* __restrict__ block_prefix, int blk, uint32_t* lds4,
                                                 int pstride = 1) {
  const int64_t base = (int64_t)blk * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  const bool full = base + SCAN_ITEMS <= n;
  if (full) {
    const uint4 a = *reinterpret_cast<const uint4*>(in + base);
    const uint4 b = *reinterpret_cast<const uint4*>(in + base + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) v[k] = (base + k < n) ? in[base + k] : 0u;
  }
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) s += v[k];
  uint32_t tot;
  uint32_t run = block_exclusive_scan_256(s, &tot, lds4) + block_prefix[(size_t)blk * pstride];
  uint32_t o[SCAN_ITEMS];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    run += v[k];
    o[k] = run;
  }
  if (full) {
    *reinterpret_cast<uint4*>(out + base) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(out + base + 4) = make_uint4(o[4], o[5], o[6], o[7]);
  } else {
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
      if (base + k < n) out[base + k] = o[k];
  }
}

