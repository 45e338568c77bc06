// ggd_mlp_wgrad.inc -- weight / bias gradients of the fused decoder (included inside ggd_mlp.hip's anonymous namespace).
//
// dW_l[out][in] = sum over points of dz_l[pt][out] * a_{l-1}[pt][in],  db_l[out] = sum_pt dz_l[pt][out],
// for the 4 layers of the 5 heads: a GEMM whose reduction index is the POINT (K = N, up to millions) and whose output is
// at most 128x128 -- split-K over the grid, fp32 MFMA accumulators per workgroup, one fp32 atomicAdd per output element
// per workgroup at the end.  HBM-bound by construction: every dz / z row (bf16) is read exactly once.
//
// Both operands come in 16-point blocks (the blocked Z layout of ggd_mlp.hip: what the forward / backward kernels produce
// with fully coalesced stores) and are streamed linearly, but an MFMA lane needs several k (= points) of ONE feature: the tiles are staged in LDS as [16-feature
// tile][64 points][16 features] sub-images and read back with the gfx950 transposing LDS load (ds_read_b64_tr_b16: a
// 16-lane group reads a [4 points][16 features] block, lane i receives the 4 points of feature i).  With that image the
// 64 lanes of one read cover 512 contiguous bytes (bank-conflict free) and every 16x16x32 fragment is two reads.
// The previous layer's activation a = gelu(z) is recomputed from the kept pre-activation while the tile is written to
// LDS (packed polynomial GELU, hidden under the HBM stream); for layer 1 the operand is the decoder input
// [plane features(32) | position(3) | earlier heads' outputs], for layer 4 the left operand is dout (fp32, 4 wide).
//
// Output (fp32, zero-initialised by the caller), WG_HEAD_FLOATS per head:
//   dW1[128][64] db1[128] dW2[128][128] db2[128] dW3[128][128] db3[128] dW4[16][128] db4[16]
constexpr int WG_K = 64;                       // points per pipeline stage
constexpr int WG_SUB = WG_K * 32 + 32;         // bytes of one [64][16] bf16 sub-image (+32 B: staggers the banks of the 8 tiles)
constexpr int WG_IMG = 8 * WG_SUB;             // one operand tile (up to 128 features)
constexpr int WG_THREADS = 512;                // 8 waves: 2 (M) x 4 (N) tiles of 64 x 32 outputs each
constexpr int WG_LDS = 4 * WG_IMG;             // A/B x double buffer = 66,560 B
constexpr int WG_OFF_W1 = 0;
constexpr int WG_OFF_B1 = WG_OFF_W1 + 128 * 64;
constexpr int WG_OFF_W2 = WG_OFF_B1 + 128;
constexpr int WG_OFF_B2 = WG_OFF_W2 + 128 * 128;
constexpr int WG_OFF_W3 = WG_OFF_B2 + 128;
constexpr int WG_OFF_B3 = WG_OFF_W3 + 128 * 128;
constexpr int WG_OFF_W4 = WG_OFF_B3 + 128;
constexpr int WG_OFF_B4 = WG_OFF_W4 + 16 * 128;
constexpr int WG_HEAD_FLOATS = WG_OFF_B4 + 16;  // 43,408

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* sub, int kb, int lane) {
  // rows kb*32 .. +15 -> k = 4g + e, rows kb*32 + 16 .. +31 -> k = 16 + 4g + e (same mapping for A and B)
  const unsigned char* p = sub + kb * 32 * 32 + lane * 8;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p + 16 * 32));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// 8 pre-activations of the forward's zbuf (f16) -> gelu(z) as the bf16 B operand
__device__ __forceinline__ uint4 gelu_bf16x8(uint4 raw) {
  const h16x8 z = __builtin_bit_cast(h16x8, raw);
  f2v gx[4] = {(f2v){(float)z[0], (float)z[1]}, (f2v){(float)z[2], (float)z[3]},
               (f2v){(float)z[4], (float)z[5]}, (f2v){(float)z[6], (float)z[7]}};
  gelu2x4(gx);
  const bf16x8 r = pack8((f4){gx[0].x, gx[0].y, gx[1].x, gx[1].y}, (f4){gx[2].x, gx[2].y, gx[3].x, gx[3].y});
  return __builtin_bit_cast(uint4, r);
}

// LAYER 1: A = dz1 [N][128], B = x0 (64 columns).   LAYER 2/3: A = dz_l, B = gelu(z_{l-1}).   LAYER 4: A = dout, B = gelu(z3).
// F16 (the reference-precision form, ggd_mlp_hl.inc): dz is the scaled fp16 plane (a slab of 32 points times 2^(4 - ks[slab])),
// z the fp16 plane, a = gelu(z) evaluated at fp32 accuracy, times 2^(ks[slab] - km), rounded to fp16; products on
// v_mfma_f32_16x16x32_f16; sums scaled by 2^(km - 4).
constexpr int HL_KNONE = -(1 << 30);   // "this slab has no gradient at this head" / "no slab has"
__device__ __forceinline__ h16x8 wg_pack8h(const f4& a, const f4& b, float k) {
  return (h16x8){h16(a[0] * k), h16(a[1] * k), h16(a[2] * k), h16(a[3] * k),
                    h16(b[0] * k), h16(b[1] * k), h16(b[2] * k), h16(b[3] * k)};
}
template <int LAYER, bool F16 = false, int CHAIN = 0 /* read by LAYER 1 only: its input columns */>
__device__ __forceinline__ void wgrad_layer(unsigned char* smem, int N, int64_t pbeg, int64_t pend,
                                            const __bf16* __restrict__ dz, const __bf16* __restrict__ zprev,
                                            const float* __restrict__ dout, const float* __restrict__ feat,
                                            const float* __restrict__ pos, const float* __restrict__ attrs,
                                            float* __restrict__ dW, float* __restrict__ db,
                                            const int* __restrict__ ks = nullptr, int km = 0,
                                            const float2* __restrict__ phi_lin = nullptr /* LDS: Phi, linear pieces */) {
  // factor of the B rows (F16): 2^(ks - km) <= 1, zero for a slab without a gradient; of layer 4's A rows: 2^(4 - ks)
  auto slab_k = [&](int64_t p) { return ks[p >> 5]; };
  auto fB = [&](int k) { return k == HL_KNONE ? 0.0f : ldexpf(1.0f, max(k - km, -80)); };
  auto fA = [&](int k) { return k == HL_KNONE ? 0.0f : ldexpf(1.0f, 4 - k); };
  const float invS = F16 ? ldexpf(1.0f, km - 4) : 1.0f;
  constexpr int MA = LAYER == 4 ? 16 : 128;          // rows of dW (output features of the layer)
  constexpr int NB = LAYER == 1 ? 64 : 128;          // columns of dW (input features)
  constexpr int WN = LAYER == 4 ? 8 : 4, WM = 8 / WN;  // wave grid
  constexpr int MT = MA / 16 / WM, NT = NB / 16 / WN;  // 16x16 tiles per wave
  constexpr int CHA = MA / 8, CHB = NB / 8;          // 16-byte chunks per point
  constexpr int TA = (WG_K * CHA + WG_THREADS - 1) / WG_THREADS;  // chunk tasks per thread
  constexpr int TB = (WG_K * CHB + WG_THREADS - 1) / WG_THREADS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv / WN, wn = wv % WN;

  f4 acc[MT][NT], bacc[MT];
#pragma unroll
  for (int a = 0; a < MT; ++a) {
    bacc[a] = (f4){0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = (f4){0, 0, 0, 0};
  }
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  auto mma = [&](const bf16x8& a, const bf16x8& b, const f4& c) {
    if constexpr (F16)
      return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
    else
      return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  };

  uint4 ra[TA];
  uint4 rb[TB];         // LAYER >= 2: raw z (bf16 x 8)
  f4 rf[TB][2];         // LAYER 1: raw fp32 input columns
  int rk[TB];           // F16: the exponent of the row's slab (raw, as loaded: turned into a factor when the stage is written,
  int ksl[2] = {HL_KNONE, HL_KNONE};   // so that load_stage never waits for a load); ksl: the exponents of the stage's two slabs

  // chunk `task` of a stage (16 bytes): for the blocked Z layout (dz, z) the stage's 64 points are four 4 KB blocks that
  // are streamed linearly; chunk -> (point inside the stage, 16-byte position q = 4k + g inside the point's row)
  auto zpt = [](int task) { return ((task >> 8) << 4) + (task & 15); };
  auto zq = [](int task) { return (task & 255) >> 4; };
  constexpr bool A_Z = LAYER != 4, B_Z = LAYER != 1;
  auto load_stage = [&](int64_t p0) {
#pragma unroll
    for (int t = 0; t < TA; ++t) {
      const int task = tid + t * WG_THREADS;
      const int pt = A_Z ? zpt(task) : task / CHA, q = A_Z ? zq(task) : task % CHA;
      const int64_t p = p0 + pt;
      ra[t] = make_uint4(0, 0, 0, 0);
      if (task < WG_K * CHA && p < pend) {
        if (LAYER == 4) {
          if (q == 0) {
            const f4 d = *reinterpret_cast<const f4*>(dout + p * 4);
            if constexpr (F16) ra[t] = __builtin_bit_cast(uint4, wg_pack8h(d, (f4){0, 0, 0, 0}, fA(slab_k(p))));
            else ra[t] = __builtin_bit_cast(uint4, pack8(d, (f4){0, 0, 0, 0}));
          }
        } else {
          ra[t] = *reinterpret_cast<const uint4*>(dz + p0 * HID + 8 * (int64_t)task);   // linear: p0 is a multiple of 16
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      const int task = tid + t * WG_THREADS;
      const int pt = B_Z ? zpt(task) : task / CHB, q = B_Z ? zq(task) : task % CHB;
      const int64_t p = p0 + pt;
      const bool ok = task < WG_K * CHB && p < pend;
      if constexpr (F16) rk[t] = ok ? slab_k(p) : HL_KNONE;
      if (LAYER == 1) {
        rf[t][0] = (f4){0, 0, 0, 0}; rf[t][1] = (f4){0, 0, 0, 0};
        if (ok) {
          if (q < 4) {
            rf[t][0] = *reinterpret_cast<const f4*>(feat + p * 32 + 8 * q);
            rf[t][1] = *reinterpret_cast<const f4*>(feat + p * 32 + 8 * q + 4);
          } else if (CHAIN == 0 && q == 4) {   // columns 32..39: position, attrs[0..4]
            const f4 a0 = *reinterpret_cast<const f4*>(attrs + p * 16);
            rf[t][0] = (f4){pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2], a0[0]};
            rf[t][1] = (f4){a0[1], a0[2], a0[3], attrs[p * 16 + 4]};
          } else if (CHAIN == 0 && q == 5) {   // columns 40..47: attrs[5..10]
            const f4 a1 = *reinterpret_cast<const f4*>(attrs + p * 16 + 4);
            const f4 a2 = *reinterpret_cast<const f4*>(attrs + p * 16 + 8);
            rf[t][0] = (f4){a1[1], a1[2], a1[3], a2[0]};
            rf[t][1] = (f4){a2[1], a2[2], 0.f, 0.f};
          } else if (CHAIN == 1 && q == 4) {   // chain 1, columns 32..39: position, attrs[11 12 13 | 8 9] (GGD_CHAIN_COL)
            const f4 a2 = *reinterpret_cast<const f4*>(attrs + p * 16 + 8);
            const f4 a3 = *reinterpret_cast<const f4*>(attrs + p * 16 + 12);
            rf[t][0] = (f4){pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2], a2[3]};
            rf[t][1] = (f4){a3[0], a3[1], a2[0], a2[1]};
          } else if (CHAIN == 1 && q == 5) {   // chain 1, columns 40..47: attrs[10 | 4 5 6 7 | 3]
            const f4 a1 = *reinterpret_cast<const f4*>(attrs + p * 16 + 4);
            rf[t][0] = (f4){attrs[p * 16 + 10], a1[0], a1[1], a1[2]};
            rf[t][1] = (f4){a1[3], attrs[p * 16 + 3], 0.f, 0.f};
          } else if (CHAIN == 2 && q == 4) {   // parallel: the position is every head's whole info vector
            rf[t][0] = (f4){pos[p * 3], pos[p * 3 + 1], pos[p * 3 + 2], 0.f};
          }
        }
      } else {
        rb[t] = make_uint4(0, 0, 0, 0);
        if (ok) rb[t] = *reinterpret_cast<const uint4*>(zprev + p0 * HID + 8 * (int64_t)task);
      }
    }
  };
  auto write_stage = [&](unsigned char* imgA, unsigned char* imgB) {
#pragma unroll
    for (int t = 0; t < TA; ++t) {
      const int task = tid + t * WG_THREADS;
      const int pt = A_Z ? zpt(task) : task / CHA, q = A_Z ? zq(task) : task % CHA;
      if (task < WG_K * CHA) *reinterpret_cast<uint4*>(imgA + (q >> 1) * WG_SUB + pt * 32 + (q & 1) * 16) = ra[t];
    }
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      const int task = tid + t * WG_THREADS;
      const int pt = B_Z ? zpt(task) : task / CHB, q = B_Z ? zq(task) : task % CHB;
      if (task < WG_K * CHB) {
        uint4 v;
        if (LAYER == 1) {
          if constexpr (F16) v = __builtin_bit_cast(uint4, wg_pack8h(rf[t][0], rf[t][1], fB(rk[t])));
          else v = __builtin_bit_cast(uint4, pack8(rf[t][0], rf[t][1]));
        } else if constexpr (F16) {
          const h16x8 z = __builtin_bit_cast(h16x8, rb[t]);
          h16x8 a;
          const float fk = fB(rk[t]);
#pragma unroll
          for (int e = 0; e < 8; ++e) { const float x = (float)z[e]; a[e] = h16((x * gt_lin<GT_N_WG>(phi_lin, x)) * fk); }
          v = __builtin_bit_cast(uint4, a);
        } else {
          v = gelu_bf16x8(rb[t]);
        }
        *reinterpret_cast<uint4*>(imgB + (q >> 1) * WG_SUB + pt * 32 + (q & 1) * 16) = v;
      }
    }
  };

  auto load_slabs = [&](int64_t p0) {   // (wave-uniform loads, raw: see rk)
    if constexpr (F16) {
      ksl[0] = p0 < pend ? slab_k(p0) : HL_KNONE;
      ksl[1] = p0 + 32 < pend ? slab_k(p0 + 32) : HL_KNONE;
    }
  };
  if (pbeg < pend) {
    load_stage(pbeg);
    load_slabs(pbeg);
    write_stage(smem, smem + WG_IMG);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t p0 = pbeg; p0 < pend; p0 += WG_K) {
    const bool more = p0 + WG_K < pend;
    const int kcur[2] = {ksl[0], ksl[1]};
    if (more) { load_stage(p0 + WG_K); load_slabs(p0 + WG_K); }
    const unsigned char* imgA = smem + buf * 2 * WG_IMG;
    const unsigned char* imgB = imgA + WG_IMG;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bf16x8 fb[NT];
      // the bias gradient's right operand: ones -- F16: times the factor of the slab these 32 points are (a stage starts on a
      // multiple of 64 points, so each half of it is exactly one slab)
      bf16x8 fone = ones;
      if constexpr (F16) {
        const _Float16 f1 = (_Float16)fB(kcur[kb]);
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f1;
        fone = __builtin_bit_cast(bf16x8, o);
      }
#pragma unroll
      for (int b = 0; b < NT; ++b) fb[b] = tr_frag(imgB + (wn * NT + b) * WG_SUB, kb, lane);
#pragma unroll
      for (int a = 0; a < MT; ++a) {
        const bf16x8 fa = tr_frag(imgA + (wm * MT + a) * WG_SUB, kb, lane);
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = mma(fa, fb[b], acc[a][b]);
        if (wn == 0) bacc[a] = mma(fa, fone, bacc[a]);
      }
    }
    buf ^= 1;
    if (more) write_stage(smem + buf * 2 * WG_IMG, smem + buf * 2 * WG_IMG + WG_IMG);
    __syncthreads();
  }
  // ---- epilogue: D layout -> lane (j, g) holds rows 16*tile + 4g + r, column 16*tile + j.  Rows that came from dz and
  //      columns that came from z are POSITIONS of the Z layout (ggd_mlp.hip): map them back to feature indices.
  auto unz = [](int p) { return (p & ~31) + ((p >> 2) & 1) * 16 + ((p >> 3) & 3) * 4 + (p & 3); };
  constexpr bool ROWS_Z = LAYER != 4, COLS_Z = LAYER != 1;
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < MT; ++a) {
    const int row0 = 16 * (wm * MT + a) + 4 * g;
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const int colp = 16 * (wn * NT + b) + j;
      const int col = COLS_Z ? unz(colp) : colp;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ROWS_Z ? unz(row0 + r) : row0 + r;
        atomicAdd(dW + (size_t)row * NB + col, F16 ? acc[a][b][r] * invS : acc[a][b][r]);
      }
    }
    if (wn == 0 && j == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(db + (ROWS_Z ? unz(row0 + r) : row0 + r), F16 ? bacc[a][r] * invS : bacc[a][r]);
    }
  }
}

template <int CHAIN>
__global__ __launch_bounds__(WG_THREADS, 4) void decoder_wgrad_kernel(
    int N, int first, int last, const __bf16* __restrict__ zbuf, const __bf16* __restrict__ dzbuf, const float* __restrict__ dout,
    const float* __restrict__ feat, const float* __restrict__ pos, const float* __restrict__ attrs,
    float* __restrict__ wgrad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int head = blockIdx.y >> 2, layer = (blockIdx.y & 3) + 1;
  const int64_t per = (((int64_t)(last - first) + gridDim.x - 1) / gridDim.x + WG_K - 1) / WG_K * WG_K;
  const int64_t pbeg = (int64_t)first + (int64_t)blockIdx.x * per;
  const int64_t pend = min((int64_t)last, pbeg + per);
  if (pbeg >= pend) return;
  float* out = wgrad + (size_t)head * WG_HEAD_FLOATS;
  const size_t LS = zlayer_elems(N);
  const __bf16* z = zbuf + (size_t)head * 3 * LS;
  const __bf16* dz = dzbuf + (size_t)head * 3 * LS;
  const float* dout_h = dout + (size_t)head * N * 4;
  switch (layer) {
    case 1: wgrad_layer<1, false, CHAIN>(smem, N, pbeg, pend, dz, nullptr, nullptr, feat, pos, attrs, out + WG_OFF_W1, out + WG_OFF_B1); break;
    case 2: wgrad_layer<2>(smem, N, pbeg, pend, dz + LS, z, nullptr, nullptr, nullptr, nullptr, out + WG_OFF_W2, out + WG_OFF_B2); break;
    case 3: wgrad_layer<3>(smem, N, pbeg, pend, dz + 2 * LS, z + LS, nullptr, nullptr, nullptr, nullptr, out + WG_OFF_W3, out + WG_OFF_B3); break;
    default: wgrad_layer<4>(smem, N, pbeg, pend, nullptr, z + 2 * LS, dout_h, nullptr, nullptr, nullptr, out + WG_OFF_W4, out + WG_OFF_B4); break;
  }
}
