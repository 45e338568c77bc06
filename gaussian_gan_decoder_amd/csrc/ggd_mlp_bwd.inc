// ggd_mlp_bwd.inc -- backward of the fused decoder (included inside ggd_mlp.hip's anonymous namespace).
//
// dL/d(activations) of the 5 heads, last head first.  Same transposed chain as the forward with the TRANSPOSED weights
// (dh_{l-1}^T = W_l^T . dz_l^T, dz_l = dh_l * gelu'(z_l)); z_l comes from the forward's zbuf.  The kernel writes
//   dzbuf[head][layer][16-point block][4 KB] (bf16, the blocked Z layout of zbuf: ggd_mlp.hip), dout[head][point][4] (fp32,
//   gradient at the head's raw 4-wide output),
// from which decoder_wgrad_kernel (ggd_mlp_wgrad.inc) forms the weight / bias gradients as [out,N]x[N,in] split-K reductions,
// accumulates dL/d(plane features) into dfeat[point][32] and carries dL/d(info) between heads in dinfo[point][16].
constexpr int ROW4T = (32 + 8) * 2;
constexpr int OFFT_W4 = 0;
constexpr int OFFT_W3 = OFFT_W4 + HID * ROW4T;
constexpr int OFFT_W2 = OFFT_W3 + HID * ROW2;
constexpr int OFFT_W1 = OFFT_W2 + HID * ROW2;
constexpr int HEADT_BYTES = OFFT_W1 + 64 * ROW2;  // 92,160 B

template <int MT, int KB, int ROW>
__device__ __forceinline__ void layer_mfma_t(const unsigned char* __restrict__ w, const bf16x8 (&bin)[2][4],
                                             f4 (&acc)[2][8], int lane) {
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    acc[0][mt] = (f4){0, 0, 0, 0}; acc[1][mt] = (f4){0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(w + wslot<ROW>(16 * mt + i, g + 4 * s));
      acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bin[0][s], acc[0][mt], 0, 0, 0);
      acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bin[1][s], acc[1][mt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// gelu'(x) = Phi(x) + x phi(x): 0.5 + xc * P7(xc^2) with xc = clamp(x, -4, 4) (least-squares fit on Chebyshev nodes, max
// |error| 3.1e-4 over all x in fp32 Horner form -- a tenth of the bf16 rounding of dz).  11 packed VALU ops per pair and no
// transcendental; the erf-polynomial + exp form it replaces cost 24 and made the kernel VALU-bound at 3.7x its MFMA time.
// Four pairs in lock step (see gelu2x4: no wait states between dependent packed ops).
__device__ __forceinline__ void gelu_grad2x4(f2v (&x)[4]) {
  f2v xc[4], s2[4], p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xc[i] = (f2v){__builtin_amdgcn_fmed3f(x[i].x, -4.0f, 4.0f), __builtin_amdgcn_fmed3f(x[i].y, -4.0f, 4.0f)};
    s2[i] = xc[i] * xc[i];
    p[i] = (f2v){-1.557768258e-08f, -1.557768258e-08f};
  }
  constexpr float C[7] = {1.163350639e-06f, -3.725065996e-05f, 6.728997635e-04f, -7.591166539e-03f,
                          5.559237280e-02f, -2.615541427e-01f, 7.965189430e-01f};
#pragma unroll
  for (int k = 0; k < 7; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = __builtin_elementwise_fma(p[i], s2[i], (f2v){C[k], C[k]});
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = __builtin_elementwise_fma(xc[i], p[i], (f2v){0.5f, 0.5f});
}

// The wave's 16 z tiles of one layer (8 bytes per lane and tile), issued BEFORE the layer's MFMAs so that the HBM
// latency is covered by them.
template <typename T, typename V8>   // (16-bit element type of the plane, its 8-vector: f16 here, opaque in ggd_mlp_hl.inc)
__device__ __forceinline__ void load_z_tiles(const T* __restrict__ zl, int64_t p0, int64_t cend, int lane,
                                             V8 (&zv)[2][4]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t pt = p0 + 16 * c + j;
    const bool ok = pt < cend;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // Z layout: tiles 2k, 2k+1 of this lane are one 16-byte piece
      zv[c][k] = __builtin_bit_cast(V8, make_uint4(0u, 0u, 0u, 0u));
      if (ok) zv[c][k] = *reinterpret_cast<const V8*>(zl + zpiece(pt, k, g));
    }
  }
}

// dz = dh * gelu'(z) for the wave's tiles, packed as the next B operand; the same 16-byte pieces are stored as dz (bf16, blocked
// Z layout).
__device__ __forceinline__ void gelu_bwd_pack(const f4 (&dh)[2][8], const h16x8 (&zv)[2][4],
                                              __bf16* __restrict__ dzl, int64_t p0, int64_t cend, int lane,
                                              bf16x8 (&bout)[2][4]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t pt = p0 + 16 * c + j;
    const bool ok = pt < cend;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      f4 out2[2];
      const h16x8 z8 = zv[c][s];   // z: f16 (the forward's own conversion, doubled)
      f2v gg[4] = {(f2v){(float)z8[0], (float)z8[1]}, (f2v){(float)z8[2], (float)z8[3]},
                   (f2v){(float)z8[4], (float)z8[5]}, (f2v){(float)z8[6], (float)z8[7]}};
      gelu_grad2x4(gg);
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int mt = 2 * s + h2;
        const f2v g0 = gg[2 * h2], g1 = gg[2 * h2 + 1];
        const f4& d = dh[c][mt];
        out2[h2] = (f4){d[0] * g0.x, d[1] * g0.y, d[2] * g1.x, d[3] * g1.y};
      }
      bout[c][s] = pack8(out2[0], out2[1]);   // the next layer's B operand AND the 16-byte Z-layout piece of dz
      if (ok) *reinterpret_cast<bf16x8*>(dzl + zpiece(pt, s, g)) = bout[c][s];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// dx = W1^T dz1 of the wave's tiles -> the gradients of the head's inputs: rows 0..31 (feature tiles 0, 1) are the plane features,
// rows 32..47 (tile 2) the info slots (position + earlier heads' outputs).  The last head (the first one the backward visits)
// writes dfeat / dinfo, every other head adds to them.
__device__ __forceinline__ void add_input_grads(const f4 (&acc)[2][8], int head, int64_t p0, int64_t cend, int lane,
                                                float* dfeat, float* dinfo) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t pt = p0 + 16 * c + j;
    if (pt >= cend) continue;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      f4* dst = reinterpret_cast<f4*>(dfeat + pt * 32 + 16 * mt + 4 * g);
      f4 v = acc[c][mt];
      if (head != NHEAD - 1) { const f4 o = *dst; v = v + o; }
      *dst = v;
    }
    f4* di = reinterpret_cast<f4*>(dinfo + pt * 16 + 4 * g);
    f4 v = acc[c][2];
    if (head != NHEAD - 1) { const f4 o = *di; v = v + o; }
    *di = v;
  }
}

// Gradient at head `head`'s raw output for one point (the lane of group 0 that owns its output rows 0..3): dattrs of the head's
// slots, plus what the later heads sent back through `info` (if the chain has a later head that reads them: chain_reads_back),
// through the derivative of the head's activation; stored to dout
// [head][point][4] (the weight-gradient kernel's layer-4 operand) and returned.
template <int CHAIN>
__device__ __forceinline__ f4 head_out_grad(int head, int64_t pt, int N, const float* __restrict__ attrs,
                                            const float* __restrict__ dattrs, const float* dinfo, float* __restrict__ dout) {
  const int attr = chain_attr(CHAIN, head);          // the attribute decoded at this position: its columns, its activation
  const int a0 = head_a0(attr), od = head_od(attr);   // first attrs slot, output width
  // where the later positions read this one's outputs: info slot 3 + its n_extra -- in chain 0 that IS a0 (said so: computed as
  // a second select chain, the chain-0 kernels come out as other code)
  const int slot = 3 + (CHAIN == 0 ? a0 : chain_nx(CHAIN, head));
  const bool back = chain_reads_back(CHAIN, head);    // does a later position read them at all?
  f4 d = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < od) {
      float v = dattrs[pt * 16 + a0 + e];
      if (!back && attr == 4) {
        v *= 0.01f;                                   // xyz = head * 0.01 + position
      } else {
        if (back) v += dinfo[pt * 16 + slot + e];     // + what the later heads sent back through `info`
        if (attr == 3) {                              // scale = -softplus(s + 5) - 2.5 (chains 1, 2: - 2)
          const float sp = -attrs[pt * 16 + a0 + e] - chain_scale_c(CHAIN);
          v *= -(1.0f - expf(-sp));                   // -sigmoid(s + 5) = -(1 - exp(-softplus))
        } else if (attr == 4) {
          v *= 0.01f;                                 // xyz as the FIRST head (chain 1): 0.01 (dattrs + dinfo)
        }
      }
      d[e] = v;
    }
  }
  *reinterpret_cast<f4*>(dout + ((size_t)head * N + pt) * 4) = d;
  return d;
}

template <int CHAIN>
__global__ __launch_bounds__(MLP_THREADS, MLP_THREADS / 256) void decoder_backward_kernel(
    int N, int first, int last, const unsigned char* __restrict__ packed_t, const float* __restrict__ attrs,
    const float* __restrict__ dattrs, const _Float16* __restrict__ zbuf, __bf16* __restrict__ dzbuf,
    float* __restrict__ dout, float* dfeat, float* dinfo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wl = smem;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  // points [first, last) of the N (N is also the row stride of the per-layer arrays)
  const int64_t per = (((int64_t)(last - first) + gridDim.x - 1) / gridDim.x + SLAB - 1) / SLAB * SLAB;
  const int64_t cbeg = (int64_t)first + (int64_t)blockIdx.x * per;
  const int64_t cend = min((int64_t)last, cbeg + per);

  for (int head = NHEAD - 1; head >= 0; --head) {
    __syncthreads();
    {
      const uint4* src = reinterpret_cast<const uint4*>(packed_t + (size_t)head * HEADT_BYTES);
      uint4* dst = reinterpret_cast<uint4*>(wl);
      for (int k = tid; k < HEADT_BYTES / 16; k += MLP_THREADS) dst[k] = src[k];
    }
    __threadfence_block();
    __syncthreads();
    const _Float16* z1 = zbuf + (size_t)(head * 3 + 0) * zlayer_elems(N);
    const _Float16* z2 = zbuf + (size_t)(head * 3 + 1) * zlayer_elems(N);
    const _Float16* z3 = zbuf + (size_t)(head * 3 + 2) * zlayer_elems(N);
    __bf16* dz1 = dzbuf + (size_t)(head * 3 + 0) * zlayer_elems(N);
    __bf16* dz2 = dzbuf + (size_t)(head * 3 + 1) * zlayer_elems(N);
    __bf16* dz3 = dzbuf + (size_t)(head * 3 + 2) * zlayer_elems(N);

    for (int64_t p0 = cbeg + (int64_t)wv * SLAB; p0 < cend; p0 += (int64_t)MLP_WAVES * SLAB) {
      // ---- gradient at the head's raw output (lane group 0 owns output rows 0..3), as the K=32 B operand
      bf16x8 bin[2][4];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int64_t pt = p0 + 16 * c + j;
        f4 d = {0, 0, 0, 0};
        if (g == 0 && pt < cend) d = head_out_grad<CHAIN>(head, pt, N, attrs, dattrs, dinfo, dout);
        const f4 z = {0, 0, 0, 0};
        bin[c][0] = pack8(d, z);
        bin[c][1] = bin[c][0]; bin[c][2] = bin[c][0]; bin[c][3] = bin[c][0];  // unused k blocks
      }
      f4 acc[2][8];
      bf16x8 bh[2][4];
      h16x8 zv[2][4];
      load_z_tiles(z3, p0, cend, lane, zv);
      layer_mfma_t<8, 1, ROW4T>(wl + OFFT_W4, bin, acc, lane);       // dh3 = W4^T dz4
      gelu_bwd_pack(acc, zv, dz3, p0, cend, lane, bh);               // dz3
      load_z_tiles(z2, p0, cend, lane, zv);
      layer_mfma_t<8, 4, ROW2>(wl + OFFT_W3, bh, acc, lane);         // dh2 = W3^T dz3
      gelu_bwd_pack(acc, zv, dz2, p0, cend, lane, bh);
      load_z_tiles(z1, p0, cend, lane, zv);
      layer_mfma_t<8, 4, ROW2>(wl + OFFT_W2, bh, acc, lane);         // dh1 = W2^T dz2
      gelu_bwd_pack(acc, zv, dz1, p0, cend, lane, bh);
      layer_mfma_t<4, 4, ROW2>(wl + OFFT_W1, bh, acc, lane);         // dx (64 input rows) = W1^T dz1
      add_input_grads(acc, head, p0, cend, lane, dfeat, dinfo);
    }
  }
}
