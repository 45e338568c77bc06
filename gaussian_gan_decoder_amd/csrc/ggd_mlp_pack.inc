// ggd_mlp_pack.inc -- builds the decoder's weight images on the device (included by ggd_mlp.hip, after ggd_mlp_hl.inc).
//
// One launch turns the 40 parameter tensors of a decoder module (per head, in the EXECUTION ORDER of its chain -- ggd_mlp.hip:
// THE THREE CHAINS; `chain` is a run-time argument here, it only sets the tensors' widths -- W1 b1 W2 b2 W3 b3 W4 b4, fp32,
// row-major [out][in] as torch.nn.Linear stores them) into the forward image (ggd_decoder_packed_bytes) and the
// transposed image the backward kernel reads (ggd_decoder_packed_t_bytes).  Training repacks after EVERY optimizer
// step; done with torch ops (pad / permute / cast / concatenate) that was ~400 tiny launches per step.
//
// Layouts of the 16-bit tier (must agree with fused_decoder.pack_weights / pack_weights_t, which remain the host-side statement
// of the format and the test's reference):
//   forward, per head : W1[128][64] W2[128][128] W3[128][128] W4[16][128] f16 (clamped to +-65504) | b1[128] b2[128] b3[128] b4[16] fp32
//                       with W1 .. W3 and b1 .. b3 HALVED: the forward's hidden accumulators hold z / 2 (ggd_mlp.hip: gelu_h2x4)
//   transposed        : W4^T[128][40] W3^T[128][128] W2^T[128][128] W1^T[64][128] bf16
// every row: K values in the MFMA operand order (inside each 32-wide k block position 8g+e holds k = 4g+e for e < 4,
// 16+4g+(e-4) otherwise), no padding (W4^T: 8 bf16 of padding), and the row's 16-byte slots XOR-swizzled by the row index
// (wslot in ggd_mlp.hip: slot q of row r sits at q ^ (r & 15) for K = 128, q ^ ((r >> 1) & 7) for K = 64; W4^T rows are
// not swizzled).  W1's K is padded from the head's in_features to 64, W4's rows from its out_features to 16 (32 in the
// transposed image's K).
// The reference-precision tier (ggd_mlp_hl.inc) has the same matrices in the same order and row format, each as TWO bf16 images,
// hi = bf16(w) then lo = bf16(w - hi), nothing halved (tests/_decoder_ref.py::pack_hl_host states it on the host):
//   forward, per head : [L1 hi | L1 lo | L2 hi | L2 lo | L3 hi | L3 lo | L4 hi | L4 lo | biases fp32]
//   transposed        : [W4^T hi | lo | W3^T hi | lo | W2^T hi | lo | W1^T hi | lo]

struct ggd_pack_ptrs { const float* p[NHEAD * 8]; };

__device__ __forceinline__ int pack_perm_col(int c) {   // source k of position c in a permuted row
  const int j = c & 31, g = j >> 3, e = j & 7;
  return (c & ~31) + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
}
// element index inside an image: logical (row r, position c) -> its swizzled slot (rows of 64 or 128 elements: wslot in
// ggd_mlp.hip); padded rows (W4^T, 40 elements) are not swizzled
__device__ __forceinline__ int pack_phys(int r, int c, int rowlen) {
  const int q = c >> 3, sw = rowlen == 128 ? (r & 15) : (rowlen == 64 ? ((r >> 1) & 7) : 0);
  return r * rowlen + ((q ^ sw) << 3) + (c & 7);
}

// One matrix of an image: `rows` rows of `rowlen` 16-bit elements, of which the first K are values (K permuted in 32-blocks).
// Element (r, k) is W[r][k] of the head's parameter tensor `src` (0: W1 [128][in_dim], 2: W2, 4: W3, 6: W4 [out_dim][128]), or
// W[k][r] in the transposed image; zero outside the tensor.  The matrices of an image follow each other in table order (an
// image of PARTS parts holds every matrix PARTS times), so the table is also the statement of the byte offsets.
struct pack_mat { int src, rows, K, rowlen; };
__device__ constexpr pack_mat PACK_MATS[2][4] = {
    {{0, HID, 64, 64}, {2, HID, HID, HID}, {4, HID, HID, HID}, {6, 16, HID, HID}},             // forward: W1 W2 W3 W4
    {{6, HID, 32, ROW4T / 2}, {4, HID, HID, HID}, {2, HID, HID, HID}, {0, 64, HID, HID}}};   // transposed: W4^T W3^T W2^T W1^T
constexpr int pack_elems(int image, int upto = 4) {   // elements of one part of the image's first `upto` matrices
  int n = 0;
  for (int m = 0; m < upto; ++m) n += PACK_MATS[image][m].rows * PACK_MATS[image][m].rowlen;
  return n;
}
constexpr int PACK_BIAS = 3 * HID + 16;
static_assert(2 * pack_elems(0, 1) == OFF_W2 && 2 * pack_elems(0, 2) == OFF_W3 && 2 * pack_elems(0, 3) == OFF_W4 &&
              2 * pack_elems(0) == OFF_B && OFF_B + 4 * PACK_BIAS == HEAD_BYTES, "forward image, 16-bit tier");
static_assert(2 * pack_elems(1, 1) == OFFT_W3 && 2 * pack_elems(1, 2) == OFFT_W2 && 2 * pack_elems(1, 3) == OFFT_W1 &&
              2 * pack_elems(1) == HEADT_BYTES, "transposed image, 16-bit tier");
static_assert(4 * pack_elems(0, 1) == HLF_L2 && 4 * pack_elems(0, 2) == HLF_L3 && 4 * pack_elems(0, 3) == HLF_L4 &&
              4 * pack_elems(0) == HLF_B && HLF_B + 4 * PACK_BIAS == HLF_HEAD && PACK_BIAS == HL_NBIAS, "forward image, split");
static_assert(4 * pack_elems(1, 1) == HLT_L3 && 4 * pack_elems(1, 2) == HLT_L2 && 4 * pack_elems(1, 3) == HLT_L1 &&
              4 * pack_elems(1) == HLT_HEAD, "transposed image, split");

// The element formats are the only per-tier code.  16-bit tier: forward f16, saturating, the hidden layers (W1 .. W3, b1 .. b3)
// HALVED -- their accumulators hold z / 2 (gelu_h2x4); transposed bf16.  HL: the bf16 hi or lo part, in both images.
template <bool HL>
__device__ __forceinline__ void pack_store(unsigned char* img, int dst, float v, bool transposed, bool hidden, bool lo) {
  if (HL) {
    const __bf16 h = (__bf16)v;
    reinterpret_cast<__bf16*>(img)[dst] = lo ? (__bf16)(v - (float)h) : h;
  } else if (transposed) {
    reinterpret_cast<__bf16*>(img)[dst] = (__bf16)v;
  } else {
    reinterpret_cast<_Float16*>(img)[dst] = h16(hidden ? 0.5f * v : v);
  }
}

// One thread per LOGICAL element of a head: [forward image: PARTS x 4 matrices | biases | transposed image: PARTS x 4 matrices]
template <bool HL>
__global__ __launch_bounds__(256) void decoder_pack_kernel(ggd_pack_ptrs ptrs, int chain, unsigned char* __restrict__ packed,
                                                           unsigned char* __restrict__ packed_t) {
  constexpr int PARTS = HL ? 2 : 1;
  constexpr int FWD = PARTS * pack_elems(0), T = PARTS * pack_elems(1), PER_HEAD = FWD + PACK_BIAS + T;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NHEAD * PER_HEAD) return;
  const int head = t / PER_HEAD;
  int e = t - head * PER_HEAD;
  const float* const* P = ptrs.p + head * 8;
  unsigned char* fwd = packed + (size_t)head * (2 * FWD + 4 * PACK_BIAS);
  if (e >= FWD && e < FWD + PACK_BIAS) {   // b1[128] b2[128] b3[128] b4[16, the head's out_dim of them]
    e -= FWD;
    float v = 0.0f;
    if (e < 3 * HID) v = (HL ? 1.0f : 0.5f) * P[1 + 2 * (e / HID)][e % HID];
    else if (e - 3 * HID < chain_od(chain, head)) v = P[7][e - 3 * HID];
    reinterpret_cast<float*>(fwd + 2 * FWD)[e] = v;
    return;
  }
  const int image = e >= FWD;
  if (image) {
    if (!packed_t) return;
    e -= FWD + PACK_BIAS;
  }
  unsigned char* img = image ? packed_t + (size_t)head * (2 * T) : fwd;
  int base = 0;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const pack_mat M = PACK_MATS[image][m];
    const int part = M.rows * M.rowlen;
    if (e < PARTS * part) {
      const bool lo = e >= part;
      const int q = lo ? e - part : e;
      const int r = q / M.rowlen, c = q - r * M.rowlen;
      float v = 0.0f;
      if (c < M.K) {
        const int k = pack_perm_col(c);
        const int out_n = M.src == 6 ? chain_od(chain, head) : HID, in_n = M.src == 0 ? chain_in(chain, head) : HID;   // the tensor is [out_n][in_n]
        const int o = image ? k : r, i = image ? r : k;
        if (o < out_n && i < in_n) v = P[M.src][o * in_n + i];
      }
      pack_store<HL>(img, base + (lo ? part : 0) + pack_phys(r, c, M.rowlen), v, image, M.src != 6, lo);
      return;
    }
    e -= PARTS * part;
    base += PARTS * part;
  }
}
