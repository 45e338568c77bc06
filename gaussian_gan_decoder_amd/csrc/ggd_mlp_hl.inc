// ggd_mlp_hl.inc -- the fused decoder at REFERENCE PRECISION on the bf16 matrix cores (included inside ggd_mlp.hip's
// anonymous namespace, after ggd_mlp_wgrad.inc; its weight images are built by ggd_mlp_pack.inc).
//
// The reference trains its decoder in fp32 (main/decoder_models/base_decoder.py:8-27).  The plain bf16 kernels round every
// weight to 8 mantissa bits -- the SAME perturbation for every point, i.e. a systematic error of the function being
// differentiated: 5-6 % in the parameter gradients.  Here every fp32 operand is split into two bf16 numbers,
//     x = hi + lo,   hi = bf16(x),   lo = bf16(x - hi)          (|x - hi - lo| <= 2^-17 |x|)
// and a product of two split operands is three MFMAs accumulated in fp32 (the lo x lo term, 2^-18 relative, is dropped):
//     W x ~= W_hi x_hi + W_hi x_lo + W_lo x_hi
//   * forward: weights AND activations split -> outputs within 1e-5 of the fp32 module; GELU = x Phi(x) with
//     Phi(-|x|) = 2^(P9(|x|/sqrt2)) / 2, P9 ~ log2 erfc (max |GELU error| 6e-7);
//   * backward: the same -- dz is split before it becomes the next MFMA operand (dX = W^T dz needs the split WEIGHTS: one
//     rounding of a weight is the same error for every point; and one bf16 for dz leaves 2^-9 of independent noise on every
//     per-point term, which does not average out of a gradient whose per-point terms have random signs -- measured 2 - 6e-3);
//   * weight gradients dW = sum over points of dz a^T, a = gelu(z): every per-point term is rounded INDEPENDENTLY, so what
//     matters is the operands' mantissa, not a split: dz is kept in HBM as ONE SCALED fp16 plane (fp16's 11-bit mantissa
//     leaves 2^-12 per term where one bf16 left 2^-9), a = gelu(z) is rounded to fp16 as well, and a product is ONE
//     v_mfma_f32_16x16x32_f16.  fp16 has 5 exponent bits and gradients have no natural scale -- here the xyz head's are 2^22
//     times the rotation head's -- so every (head, 32-point slab) carries its own power-of-two scale 2^(4 - e), e the
//     exponent of the slab's largest gradient at that head's output (so that it lands in [8, 16): 2^12 of headroom for what
//     the weights' row sums can add from layer to layer, saturating beyond; 2^18 down to fp16's subnormals).  The backward
//     stores e per (head, slab) and the largest e per head; the weight-gradient kernel multiplies a slab's `a` rows by
//     2^(e - e_max) <= 1 in fp32 before rounding them (a slab 2^14 below the head's largest drops out: its terms are below
//     the sums' own rounding) and the sums by 2^(e_max - 4).  (Round 3 kept dz as two bf16 planes and multiplied split
//     operands, three MFMAs per product: 23 GB instead of 15 GB per weight-gradient pass at 2 M points.)
//   * z is kept in HBM as ONE fp16 plane: it only enters through gelu'(z) and a = gelu(z), where 11 mantissa bits leave
//     <= 2e-4 relative error per element; pre-activations sit comfortably inside fp16's range, and one that does not is
//     clamped to +-65504 (gelu' is 0 / 1 there either way).  The decoder kernels are bound by this traffic (two full bf16
//     planes for z cost 30 % more time).
// Split weights of one head are 168 KB -- more than the CU's 160 KB of LDS -- so the weights are CYCLED layer by layer
// through two 64 KB LDS buffers: while the workgroup's 8 waves run layer l out of one buffer, layer l + 1 (hi and lo
// images, contiguous in the packed array) streams from L2 into the other with LDS-direct loads (global_load_lds_dwordx4:
// no registers, no VALU), one workgroup barrier per layer.  Re-reading 0.9 MB of weights per 256 points costs ~10 % of
// the CU's L2 bandwidth.  All biases (8 KB) are resident.

constexpr int HL_P1 = HID * ROW1;                 // 16,384 B: one part (hi or lo) of layer 1 [128][64]
constexpr int HL_P2 = HID * ROW2;                 // 32,768 B: layers 2, 3 [128][128]
constexpr int HL_P4 = 16 * ROW2;                  //  4,096 B: layer 4 [16][128]
constexpr int HLF_L1 = 0;
constexpr int HLF_L2 = HLF_L1 + 2 * HL_P1;
constexpr int HLF_L3 = HLF_L2 + 2 * HL_P2;
constexpr int HLF_L4 = HLF_L3 + 2 * HL_P2;
constexpr int HLF_B = HLF_L4 + 2 * HL_P4;         // fp32 biases b1[128] b2[128] b3[128] b4[16]
constexpr int HL_NBIAS = 3 * HID + 16;
constexpr int HLF_HEAD = HLF_B + HL_NBIAS * 4;    // 173,632 B per head
constexpr int HL_PT4 = HID * ROW4T;               // 10,240 B: W4^T [128][40]
constexpr int HL_PT1 = 64 * ROW2;                 // 16,384 B: W1^T [64][128]
constexpr int HLT_L4 = 0;
constexpr int HLT_L3 = HLT_L4 + 2 * HL_PT4;
constexpr int HLT_L2 = HLT_L3 + 2 * HL_P2;
constexpr int HLT_L1 = HLT_L2 + 2 * HL_P2;
constexpr int HLT_HEAD = HLT_L1 + 2 * HL_PT1;     // 184,320 B per head
constexpr int HL_BUF = 2 * HL_P2;                 // 65,536 B: one LDS weight buffer (the largest layer, hi + lo)
constexpr int HL_LDS_FWD = 2 * HL_BUF + NHEAD * HL_NBIAS * 4 + gt_bytes(GT_N_FWD);   // 139,072 B + the Phi table (16,400 B)
constexpr int HL_LDS_BWD = 2 * HL_BUF + gt_bytes(GT_N_BWD);                          // + the gelu' table (32,768 B): all 160 KB
constexpr int WGH_LDS = WG_LDS + gt_bytes(GT_N_WG);                                  // weight gradients: + Phi (two workgroups per CU still fit)
static_assert(HL_LDS_BWD <= 160 * 1024 && HL_LDS_FWD <= 160 * 1024, "LDS budget");
static_assert((2 * HL_P1) % 1024 == 0 && (2 * HL_P2) % 1024 == 0 && (2 * HL_P4) % 1024 == 0 && (2 * HL_PT4) % 1024 == 0 &&
              (2 * HL_PT1) % 1024 == 0, "a wave's LDS-direct load covers 1 KB");

// One wave instruction: lane l copies the 16 bytes at ITS global address to LDS[lds_off + 16 l] (M0 = the wave's LDS
// destination).  Through inline asm so that the compiler does not serialise the stream against the LDS reads of the layer
// being computed (it cannot tell the two weight buffers apart inside one dynamic LDS array and would wait for every
// LDS-direct load before the next ds_read); the consumer side waits explicitly, see hl_step_begin.
__device__ __forceinline__ void hl_dma16(const void* gptr, uint32_t lds_off) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" :: "s"(lds_off), "v"(gptr) : "memory");
}
// the workgroup's NW waves stream `bytes` (a multiple of 1024) from src to LDS offset dst
template <int NW>
__device__ __forceinline__ void hl_stream(const unsigned char* __restrict__ src, uint32_t dst, int bytes, int wv, int lane) {
  for (int off = wv * 1024; off < bytes; off += NW * 1024)
    hl_dma16(src + off + lane * 16, (uint32_t)__builtin_amdgcn_readfirstlane((int)(dst + off)));
}
// Top of a layer step: this wave's LDS-direct loads (and everything else it has outstanding) have landed, then the
// workgroup barrier: every wave's share of the layer's weights is in LDS, and every wave has finished reading the OTHER
// buffer, which the caller now refills.
__device__ __forceinline__ void hl_step_begin() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// 8 fp32 values -> their bf16 hi and lo parts (the B-operand pieces of the next layer)
__device__ __forceinline__ void split8(const f4& a, const f4& b, bf16x8& hi, bf16x8& lo) {
  hi = pack8(a, b);
  const f4 ra = {a[0] - (float)hi[0], a[1] - (float)hi[1], a[2] - (float)hi[2], a[3] - (float)hi[3]};
  const f4 rb = {b[0] - (float)hi[4], b[1] - (float)hi[5], b[2] - (float)hi[6], b[3] - (float)hi[7]};
  lo = pack8(ra, rb);
}

// One layer on split operands for the wave's two 16-point column tiles, MT feature tiles of 16 rows:
//   acc[c][mt] = (BIAS ? bias : 0) + W_lo x_hi + W_hi x_lo + W_hi x_hi       (three MFMAs per fragment pair, small terms first)
// forward: x = the activations, W a hidden layer (MT = 8, BIAS); backward: x = dz, W a transposed layer (dh = W^T dz, no bias).
// w: the layer's hi image, the lo image PART bytes behind it.
template <int MT, int KB, int ROW, int PART, bool BIAS>
__device__ __forceinline__ void layer_mfma_hl(const unsigned char* __restrict__ w, const float* __restrict__ bias,
                                              const bf16x8 (&bhi)[2][4], const bf16x8 (&blo)[2][4], f4 (&acc)[2][8],
                                              int lane) {
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    // (no look-ahead on the weight fragments here: hi + lo fragments of two tiles would not fit the 256 registers a wave
    // has at two waves per SIMD; the six MFMAs per fragment pair and the SIMD's other wave cover the LDS latency)
    bf16x8 ah[KB], al[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      const int o = wslot<ROW>(16 * mt + i, g + 4 * s);
      ah[s] = *reinterpret_cast<const bf16x8*>(w + o);
      al[s] = *reinterpret_cast<const bf16x8*>(w + PART + o);
    }
    f4 bb = {0, 0, 0, 0};
    if (BIAS) bb = *reinterpret_cast<const f4*>(bias + 16 * mt + 4 * g);
    acc[0][mt] = bb; acc[1][mt] = bb;
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[s], bhi[0][s], acc[0][mt], 0, 0, 0);
      acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[s], bhi[1][s], acc[1][mt], 0, 0, 0);
      acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[s], blo[0][s], acc[0][mt], 0, 0, 0);
      acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[s], blo[1][s], acc[1][mt], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[s], bhi[0][s], acc[0][mt], 0, 0, 0);
      acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[s], bhi[1][s], acc[1][mt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// z of the wave's tiles as fp16 pieces (blocked Z layout, zpiece: the positions and 16-byte pieces of gelu_pack's stores).  The stores are
// DEFERRED to the top of the next layer step: a step begins by waiting for everything the wave has outstanding (that is how
// the LDS-direct weight loads are awaited: loads and stores share one counter and complete out of order with respect to each
// other), and stores issued at the end of the previous step would put an HBM write round trip on that wait (measured: 23 k
// cycles per step with them, against ~8 k of MFMA + GELU work).  Issued right after the wait they have a whole step to land.
__device__ __forceinline__ void pack_z16(const f4 (&acc)[2][8], h16x8 (&zr)[2][4]) {
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f4& a0 = acc[c][2 * k];
      const f4& a1 = acc[c][2 * k + 1];
      zr[c][k] = (h16x8){h16(a0[0]), h16(a0[1]), h16(a0[2]), h16(a0[3]), h16(a1[0]), h16(a1[1]), h16(a1[2]), h16(a1[3])};
    }
}
__device__ __forceinline__ void flush_z16(_Float16* __restrict__ zl, const h16x8 (&zr)[2][4], int64_t p0, int64_t cend,
                                          int lane) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t pt = p0 + 16 * c + j;
    if (pt >= cend) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<h16x8*>(zl + zpiece(pt, k, g)) = zr[c][k];
  }
}

// GELU of the wave's tiles at fp32 accuracy, split into the next layer's hi / lo B operands
__device__ __forceinline__ void gelu_split(const f4 (&acc)[2][8], bf16x8 (&ohi)[2][4], bf16x8 (&olo)[2][4], uint32_t phi_lds) {
  float sc = (float)GT_N_FWD / 12.0f, hf = 0.5f * (float)GT_N_FWD, hi = (float)GT_N_FWD - 0.001f;
  asm volatile("" : "+v"(sc), "+v"(hf), "+v"(hi));   // (VGPR operands of the look-up block)
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const f4& a0 = acc[c][2 * s];
      const f4& a1 = acc[c][2 * s + 1];
      float p0 = a0[0], p1 = a0[1], p2 = a0[2], p3 = a0[3], p4 = a1[0], p5 = a1[1], p6 = a1[2], p7 = a1[3];   // -> Phi(x)
      gt_lin4(phi_lds, sc, hf, hi, p0, p1, p2, p3);
      gt_lin4(phi_lds, sc, hf, hi, p4, p5, p6, p7);
      const f4 g0 = {a0[0] * p0, a0[1] * p1, a0[2] * p2, a0[3] * p3};      // gelu = x Phi(x)
      const f4 g1 = {a1[0] * p4, a1[1] * p5, a1[2] * p6, a1[3] * p7};
      split8(g0, g1, ohi[c][s], olo[c][s]);
      __builtin_amdgcn_sched_barrier(0);
    }
}

// Forward.  Same point / wave / register mapping as decoder_forward_kernel (32-point slabs, D layout of a layer == B
// layout of the next); the loop nest is batch (256 points per workgroup) -> head -> layer, with the layer's weights in
// buffer (layer - 1) % 2 and the next step's weights streaming into the other one.
template <int CHAIN, bool STORE_Z>
__global__ __launch_bounds__(FWD_THREADS) void decoder_forward_hl_kernel(const float* __restrict__ feat,
                                                                         const float* __restrict__ pos, int N,
                                                                         const unsigned char* __restrict__ packed,
                                                                         float* attrs, __bf16* __restrict__ zbuf,
                                                                         const unsigned char* __restrict__ gtab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* buf0 = smem;
  unsigned char* buf1 = smem + HL_BUF;
  float* biases = reinterpret_cast<float*>(smem + 2 * HL_BUF);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const uint32_t phi_tbl = lds0 + 2 * HL_BUF + NHEAD * HL_NBIAS * 4;   // LDS byte address of the Phi table
  const uint32_t lds1 = lds0 + HL_BUF;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  constexpr int BATCH = FWD_WAVES * SLAB;

  const int64_t per = (((int64_t)N + gridDim.x - 1) / gridDim.x + BATCH - 1) / BATCH * BATCH;
  const int64_t cbeg = (int64_t)blockIdx.x * per;
  const int64_t cend = min((int64_t)N, cbeg + per);
  if (cbeg >= cend) return;                                   // workgroup-uniform
  const int nbatch = (int)((cend - cbeg + BATCH - 1) / BATCH);

  gt_load(smem + 2 * HL_BUF + NHEAD * HL_NBIAS * 4, gtab + GT_OFF_FWD, gt_bytes(GT_N_FWD), tid, FWD_THREADS);   // (the first layer
  for (int k = tid; k < NHEAD * HL_NBIAS; k += FWD_THREADS) {                                                  // step's barrier covers it)
    const int h = k / HL_NBIAS, e = k - h * HL_NBIAS;
    biases[k] = reinterpret_cast<const float*>(packed + (size_t)h * HLF_HEAD + HLF_B)[e];
  }
  hl_stream<FWD_WAVES>(packed + HLF_L1, lds0, 2 * HL_P1, wv, lane);        // step 0: head 0, layer 1 -> buffer 0

  for (int b = 0; b < nbatch; ++b) {
    const int64_t p0 = cbeg + (int64_t)b * BATCH + (int64_t)wv * SLAB;
    for (int head = 0; head < NHEAD; ++head) {
      const int n_extra = GGD_CHAIN_NX(CHAIN, head);   // = chain_nx(CHAIN, head), expanded in place
      const unsigned char* hw = packed + (size_t)head * HLF_HEAD;
      const float* b1 = biases + head * HL_NBIAS;
      const float* b2 = b1 + HID;
      const float* b3 = b2 + HID;
      const float* b4 = b3 + HID;
      // ---- inputs, split: k-block 0 = 32 plane features, k-block 1 = info slots 4g..4g+3 (upper half of the block zero)
      bf16x8 bhi[2][4], blo[2][4];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int64_t pt = p0 + 16 * c + j;
        const bool ok = pt < cend;
        f4 lo4 = {0, 0, 0, 0}, hi4 = {0, 0, 0, 0}, inf = {0, 0, 0, 0};
        if (ok) {
          lo4 = *reinterpret_cast<const f4*>(feat + pt * 32 + 4 * g);
          hi4 = *reinterpret_cast<const f4*>(feat + pt * 32 + 16 + 4 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int q = 4 * g + e;  // info slot
            float v = 0.0f;
            if (q < 3) v = pos[pt * 3 + q];
            else if (q - 3 < n_extra) {
              int col = GGD_CHAIN_COL(CHAIN, q - 3);
              // (chain 1's four columns are four addresses per point tile, the same for every head: left alone they are
              // hoisted out of the head loop and spilled -- 18 VGPRs in decoder_forward_hl_kernel<1, true>; opaque, they are
              // formed again from the row's address where they are used)
              if (CHAIN == 1) asm volatile("" : "+v"(col));
              v = attrs[pt * 16 + col];
            }
            inf[e] = v;
          }
        }
        const f4 z = {0, 0, 0, 0};
        split8(lo4, hi4, bhi[c][0], blo[c][0]);
        split8(inf, z, bhi[c][1], blo[c][1]);
        bhi[c][2] = bhi[c][1]; bhi[c][3] = bhi[c][1]; blo[c][2] = blo[c][1]; blo[c][3] = blo[c][1];   // unused k blocks
      }
      f4 acc[2][8];
      h16x8 zr[2][4];      // the layer's z as fp16, stored at the top of the NEXT step (see pack_z16)
      _Float16* zh = reinterpret_cast<_Float16*>(zbuf) + (size_t)(head * 3) * zlayer_elems(N);
      // ---- layer 1 (buffer 0); layer 2 streams into buffer 1
      hl_step_begin();
      hl_stream<FWD_WAVES>(hw + HLF_L2, lds1, 2 * HL_P2, wv, lane);
      layer_mfma_hl<8, 2, ROW1, HL_P1, true>(buf0, b1, bhi, blo, acc, lane);
      if (STORE_Z) pack_z16(acc, zr);
      gelu_split(acc, bhi, blo, phi_tbl);
      // ---- layer 2 (buffer 1); layer 3 streams into buffer 0
      hl_step_begin();
      hl_stream<FWD_WAVES>(hw + HLF_L3, lds0, 2 * HL_P2, wv, lane);
      if (STORE_Z) flush_z16(zh, zr, p0, cend, lane);
      layer_mfma_hl<8, 4, ROW2, HL_P2, true>(buf1, b2, bhi, blo, acc, lane);
      if (STORE_Z) pack_z16(acc, zr);
      gelu_split(acc, bhi, blo, phi_tbl);
      // ---- layer 3 (buffer 0); layer 4 streams into buffer 1
      hl_step_begin();
      hl_stream<FWD_WAVES>(hw + HLF_L4, lds1, 2 * HL_P4, wv, lane);
      if (STORE_Z) flush_z16(zh + zlayer_elems(N), zr, p0, cend, lane);
      layer_mfma_hl<8, 4, ROW2, HL_P2, true>(buf0, b3, bhi, blo, acc, lane);
      if (STORE_Z) pack_z16(acc, zr);
      gelu_split(acc, bhi, blo, phi_tbl);
      // ---- output layer (buffer 1): one feature tile; the next step's layer 1 (next head, or head 0 of the next batch)
      //      streams into buffer 0
      hl_step_begin();
      if (STORE_Z) flush_z16(zh + 2 * zlayer_elems(N), zr, p0, cend, lane);
      {
        const int nh = head + 1 < NHEAD ? head + 1 : 0;
        if (head + 1 < NHEAD || b + 1 < nbatch)
          hl_stream<FWD_WAVES>(packed + (size_t)nh * HLF_HEAD + HLF_L1, lds0, 2 * HL_P1, wv, lane);
      }
      f4 out[2];
      {
        const f4 bb = *reinterpret_cast<const f4*>(b4 + 4 * g);
        out[0] = bb; out[1] = bb;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int o = wslot<ROW2>(j, g + 4 * s);
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(buf1 + o);
          const bf16x8 al = *reinterpret_cast<const bf16x8*>(buf1 + HL_P4 + o);
          out[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bhi[0][s], out[0], 0, 0, 0);
          out[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bhi[1][s], out[1], 0, 0, 0);
          out[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, blo[0][s], out[0], 0, 0, 0);
          out[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, blo[1][s], out[1], 0, 0, 0);
          out[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bhi[0][s], out[0], 0, 0, 0);
          out[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bhi[1][s], out[1], 0, 0, 0);
        }
      }
      const int attr = GGD_CHAIN_ATTR(CHAIN, head);   // the attribute this position decodes (see decoder_forward_kernel)
      if (g == 0) {   // lane group 0 holds output features 0..3 of point j (D rows 0..3)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int64_t pt = p0 + 16 * c + j;
          if (pt >= cend) continue;
          float* arow = attrs + pt * 16;
          const f4 o = out[c];
          if (attr == 0) {
            arow[0] = o[0]; arow[1] = o[1]; arow[2] = o[2];
          } else if (attr == 1) {
            arow[3] = o[0];
          } else if (attr == 2) {
            arow[4] = o[0]; arow[5] = o[1]; arow[6] = o[2]; arow[7] = o[3];
          } else if (attr == 3) {  // -softplus(s + 5) - 2.5, or - 2 (chain_scale_c)   (torch.nn.Softplus: beta 1, threshold 20)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              const float v = o[q] + 5.0f;
              const float sp = v > 20.0f ? v : __logf(1.0f + __expf(v));   // <= 2e-7 absolute (see decoder_forward_kernel); this tier's bar is 1e-4
              arow[8 + q] = -sp - chain_scale_c(CHAIN);
            }
          } else {                 // xyz = head * 0.01 + position
            arow[11] = o[0] * 0.01f + pos[pt * 3]; arow[12] = o[1] * 0.01f + pos[pt * 3 + 1];
            arow[13] = o[2] * 0.01f + pos[pt * 3 + 2];
            arow[14] = 0.0f; arow[15] = 0.0f;
          }
        }
      }
    }
  }
}

// dz = dh * gelu'(z) for the wave's tiles at fp32 accuracy (z: the fp16 plane, raw 16-byte pieces as load_z_tiles returns
// them), split into hi / lo parts, the next layer's B operands; and dz * S as ONE fp16 plane (dzs), which flush_z16
// writes at the top of the next step (deferred like the forward's z stores).
__device__ __forceinline__ void gelu_bwd_split(const f4 (&dh)[2][8], const bf16x8 (&zraw)[2][4],
                                               bf16x8 (&ohi)[2][4], bf16x8 (&olo)[2][4], h16x8 (&dzs)[2][4], float S,
                                               uint32_t dg_lds) {
  float sc = (float)GT_N_BWD / 12.0f, hf = 0.5f * (float)GT_N_BWD, hi = (float)GT_N_BWD - 0.001f;
  asm volatile("" : "+v"(sc), "+v"(hf), "+v"(hi));
#pragma unroll
  for (int c = 0; c < 2; ++c) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const h16x8 z8 = __builtin_bit_cast(h16x8, zraw[c][s]);
      f4 out2[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const f4& d = dh[c][2 * s + h2];
        float q0 = (float)z8[4 * h2], q1 = (float)z8[4 * h2 + 1], q2 = (float)z8[4 * h2 + 2], q3 = (float)z8[4 * h2 + 3];   // -> gelu'(z)
        gt_lin4(dg_lds, sc, hf, hi, q0, q1, q2, q3);
        out2[h2] = (f4){d[0] * q0, d[1] * q1, d[2] * q2, d[3] * q3};
      }
      split8(out2[0], out2[1], ohi[c][s], olo[c][s]);
      dzs[c][s] = (h16x8){h16(out2[0][0] * S), h16(out2[0][1] * S), h16(out2[0][2] * S), h16(out2[0][3] * S),
                          h16(out2[1][0] * S), h16(out2[1][1] * S), h16(out2[1][2] * S), h16(out2[1][3] * S)};
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// Backward on split operands: the loop nest of decoder_backward_kernel turned batch -> head (last first) -> layer (last
// first), weights cycled as in the forward: W4^T -> buffer 0, W3^T -> 1, W2^T -> 0, W1^T -> 1.
template <int CHAIN>
__global__ __launch_bounds__(MLP_THREADS) void decoder_backward_hl_kernel(
    int N, int first, int last, const unsigned char* __restrict__ packed_t, const float* __restrict__ attrs,
    const float* __restrict__ dattrs, const __bf16* __restrict__ zbuf, __bf16* __restrict__ dzbuf,
    float* __restrict__ dout, float* dfeat, float* dinfo, int* __restrict__ karr /* [NHEAD][slabs] */,
    int* __restrict__ kref /* [NHEAD] */, const unsigned char* __restrict__ gtab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* buf0 = smem;
  unsigned char* buf1 = smem + HL_BUF;
  gt_load(smem + 2 * HL_BUF, gtab + GT_OFF_BWD, gt_bytes(GT_N_BWD), threadIdx.x, MLP_THREADS);   // (covered by the first step's barrier)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const uint32_t lds1 = lds0 + HL_BUF;
  const uint32_t dg_tbl = lds0 + 2 * HL_BUF;                           // LDS byte address of the gelu' table
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  constexpr int BATCH = MLP_WAVES * SLAB;
  const int64_t per = (((int64_t)(last - first) + gridDim.x - 1) / gridDim.x + BATCH - 1) / BATCH * BATCH;
  const int64_t cbeg = (int64_t)first + (int64_t)blockIdx.x * per;
  const int64_t cend = min((int64_t)last, cbeg + per);
  if (cbeg >= cend) return;
  const int nbatch = (int)((cend - cbeg + BATCH - 1) / BATCH);
  const size_t LS = zlayer_elems(N);   // dzbuf: one scaled fp16 plane; zbuf: one fp16 plane
  const int64_t nslab = ((int64_t)N + SLAB - 1) / SLAB;

  hl_stream<MLP_WAVES>(packed_t + (size_t)(NHEAD - 1) * HLT_HEAD + HLT_L4, lds0, 2 * HL_PT4, wv, lane);   // step 0

  for (int b = 0; b < nbatch; ++b) {
    const int64_t p0 = cbeg + (int64_t)b * BATCH + (int64_t)wv * SLAB;
    for (int head = NHEAD - 1; head >= 0; --head) {
      const unsigned char* hw = packed_t + (size_t)head * HLT_HEAD;
      const __bf16* z1 = zbuf + (size_t)(head * 3 + 0) * LS;
      const __bf16* z2 = zbuf + (size_t)(head * 3 + 1) * LS;
      const __bf16* z3 = zbuf + (size_t)(head * 3 + 2) * LS;
      _Float16* dz1 = reinterpret_cast<_Float16*>(dzbuf) + (size_t)(head * 3 + 0) * LS;
      _Float16* dz2 = reinterpret_cast<_Float16*>(dzbuf) + (size_t)(head * 3 + 1) * LS;
      _Float16* dz3 = reinterpret_cast<_Float16*>(dzbuf) + (size_t)(head * 3 + 2) * LS;
      // ---- gradient at the head's raw output (lane group 0 owns output rows 0..3), as the K = 32 B operand (split)
      bf16x8 bhi[2][4], blo[2][4];
      float dmax = 0.0f;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int64_t pt = p0 + 16 * c + j;
        f4 d = {0, 0, 0, 0};
        if (g == 0 && pt < cend) d = head_out_grad<CHAIN>(head, pt, N, attrs, dattrs, dinfo, dout);
        const f4 z = {0, 0, 0, 0};
        split8(d, z, bhi[c][0], blo[c][0]);
        bhi[c][1] = bhi[c][0]; bhi[c][2] = bhi[c][0]; bhi[c][3] = bhi[c][0];  // unused k blocks
        blo[c][1] = blo[c][0]; blo[c][2] = blo[c][0]; blo[c][3] = blo[c][0];
        dmax = fmaxf(dmax, fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fmaxf(fabsf(d[2]), fabsf(d[3]))));
      }
      // the slab's scale for this head's dz planes: largest |gradient at the head's output| -> [8, 16)
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, sh, 64));
      int ke = HL_KNONE;
      float S = 1.0f;
      if (dmax > 0.0f && dmax <= 3.0e38f) { (void)frexpf(dmax, &ke); S = ldexpf(1.0f, 4 - ke); }
      if (lane == 0 && p0 < cend) {
        karr[(size_t)head * nslab + p0 / SLAB] = ke;
        if (ke != HL_KNONE) atomicMax(&kref[head], ke);
      }
      f4 acc[2][8];
      bf16x8 zv[2][4];   // raw 16-byte pieces of the fp16 z plane
      h16x8 dzs[2][4];   // the layer's dz * S as fp16, stored at the top of the NEXT step
      // ---- dh3 = W4^T dz4 (buffer 0); W3^T streams into buffer 1
      hl_step_begin();
      hl_stream<MLP_WAVES>(hw + HLT_L3, lds1, 2 * HL_P2, wv, lane);
      load_z_tiles(z3, p0, cend, lane, zv);
      layer_mfma_hl<8, 1, ROW4T, HL_PT4, false>(buf0, nullptr, bhi, blo, acc, lane);
      gelu_bwd_split(acc, zv, bhi, blo, dzs, S, dg_tbl);
      // ---- dh2 = W3^T dz3 (buffer 1); W2^T -> buffer 0
      hl_step_begin();
      hl_stream<MLP_WAVES>(hw + HLT_L2, lds0, 2 * HL_P2, wv, lane);
      flush_z16(dz3, dzs, p0, cend, lane);
      load_z_tiles(z2, p0, cend, lane, zv);
      layer_mfma_hl<8, 4, ROW2, HL_P2, false>(buf1, nullptr, bhi, blo, acc, lane);
      gelu_bwd_split(acc, zv, bhi, blo, dzs, S, dg_tbl);
      // ---- dh1 = W2^T dz2 (buffer 0); W1^T -> buffer 1
      hl_step_begin();
      hl_stream<MLP_WAVES>(hw + HLT_L1, lds1, 2 * HL_PT1, wv, lane);
      flush_z16(dz2, dzs, p0, cend, lane);
      load_z_tiles(z1, p0, cend, lane, zv);
      layer_mfma_hl<8, 4, ROW2, HL_P2, false>(buf0, nullptr, bhi, blo, acc, lane);
      gelu_bwd_split(acc, zv, bhi, blo, dzs, S, dg_tbl);
      // ---- dx (64 input rows) = W1^T dz1 (buffer 1); the next step's W4^T (head - 1, or the last head of the next batch)
      //      streams into buffer 0
      hl_step_begin();
      flush_z16(dz1, dzs, p0, cend, lane);
      {
        const int nh = head > 0 ? head - 1 : NHEAD - 1;
        if (head > 0 || b + 1 < nbatch)
          hl_stream<MLP_WAVES>(packed_t + (size_t)nh * HLT_HEAD + HLT_L4, lds0, 2 * HL_PT4, wv, lane);
      }
      layer_mfma_hl<4, 4, ROW2, HL_PT1, false>(buf1, nullptr, bhi, blo, acc, lane);
      add_input_grads(acc, head, p0, cend, lane, dfeat, dinfo);
    }
  }
}

// ---- weight / bias gradients at reference precision --------------------------------------------------------------------------
// wgrad_layer<LAYER, true> (ggd_mlp_wgrad.inc) on fp16 operands: A = the scaled fp16 dz plane the backward wrote, streamed into
// LDS untouched (layer 4: dout * 2^(4 - e)); B = gelu(z) at fp32 accuracy from the fp16 z plane, times the slab's 2^(e - e_max),
// rounded to fp16 (layer 1: the fp32 decoder inputs); one v_mfma_f32_16x16x32_f16 per product, 2^(e_max - 4) applied to the
// sums in the epilogue.
template <int CHAIN>
__global__ __launch_bounds__(WG_THREADS, 4) void decoder_wgrad_hl_kernel(
    int N, int first, int last, const __bf16* __restrict__ zbuf, const __bf16* __restrict__ dzbuf, const float* __restrict__ dout,
    const float* __restrict__ feat, const float* __restrict__ pos, const float* __restrict__ attrs,
    float* __restrict__ wgrad, const int* __restrict__ karr, const int* __restrict__ kref,
    const unsigned char* __restrict__ gtab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int head = blockIdx.y >> 2, layer = (blockIdx.y & 3) + 1;
  const float2* phi_lin = reinterpret_cast<const float2*>(smem + WG_LDS);
  const int64_t per = (((int64_t)(last - first) + gridDim.x - 1) / gridDim.x + WG_K - 1) / WG_K * WG_K;
  const int64_t pbeg = (int64_t)first + (int64_t)blockIdx.x * per;
  const int64_t pend = min((int64_t)last, pbeg + per);
  if (pbeg >= pend) return;
  const int km = kref[head];
  if (km < HL_KNONE) return;
  if (layer != 1) {   // (layer 1's right operand is the decoder input, no GELU)
    gt_load(smem + WG_LDS, gtab + GT_OFF_WG, gt_bytes(GT_N_WG), threadIdx.x, WG_THREADS);
    __syncthreads();
  }           // still the memset pattern: no slab of this head had a gradient, dW stays zero
  float* out = wgrad + (size_t)head * WG_HEAD_FLOATS;
  const size_t LS = zlayer_elems(N);
  const __bf16* z = zbuf + (size_t)head * 3 * LS;
  const __bf16* dz = dzbuf + (size_t)head * 3 * LS;
  const float* dout_h = dout + (size_t)head * N * 4;
  const int* ks = karr + (size_t)head * (((int64_t)N + SLAB - 1) / SLAB);
  switch (layer) {
    case 1: wgrad_layer<1, true, CHAIN>(smem, N, pbeg, pend, dz, nullptr, nullptr, feat, pos, attrs, out + WG_OFF_W1, out + WG_OFF_B1, ks, km, phi_lin); break;
    case 2: wgrad_layer<2, true>(smem, N, pbeg, pend, dz + LS, z, nullptr, nullptr, nullptr, nullptr, out + WG_OFF_W2, out + WG_OFF_B2, ks, km, phi_lin); break;
    case 3: wgrad_layer<3, true>(smem, N, pbeg, pend, dz + 2 * LS, z + LS, nullptr, nullptr, nullptr, nullptr, out + WG_OFF_W3, out + WG_OFF_B3, ks, km, phi_lin); break;
    default: wgrad_layer<4, true>(smem, N, pbeg, pend, nullptr, z + 2 * LS, dout_h, nullptr, nullptr, nullptr, out + WG_OFF_W4, out + WG_OFF_B4, ks, km, phi_lin); break;
  }
}
