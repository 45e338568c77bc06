// ggd_perceptual.hip -- the perceptual term (losses.PerceptualStandIn: a VGG16-shaped trunk, five channel-normalised taps,
// squared distance) on the device: forward of image and target as one batch, the loss, and the gradient into the image.
//
// Layout: activations are NHWC ([pixel][channel], pixel = (b, y, x) row-major), so the K slice of one filter tap is a run of
// contiguous channels.  Storage type per tier (ggd_perceptual_desc::tier):
//   GGD_PERC_BF16   forward activations f16 (clamped to +-65504), gradients bf16; one MFMA per product
//   GGD_PERC_FP32   both fp32 words that hold hi + lo of a split-bf16 pair exactly (round_split); the convolution splits them
//                   again on the way into LDS and spends three MFMAs per product (hi*hi + lo*hi + hi*lo)
// Kernels:
//   perc_prologue / perc_prologue_bwd   per-channel affine + kh x kw mean, NCHW fp32 <-> NHWC fp32
//   perc_conv0_fwd / perc_conv0_bwd     conv1_1 (3 -> C0) and its backward to the image in fp32 FMA
//   perc_conv<T, CT, EPI>               the other twelve convolutions and their backward-data passes: implicit GEMM on
//                                       v_mfma_f32_16x16x32_{f16,bf16}.  C^T = W^T X^T: the weights are the A operand (rows = output
//                                       channels), the pixels the B operand (columns), so a lane ends with 4 consecutive channels of one
//                                       pixel.  Block = 128 pixels x 32 CT channels, 4 waves as 2 x 2, K step = (tap, 32 channels); the
//                                       pixel tile goes global -> registers -> LDS (predicated: zero padding), the weights are
//                                       pre-packed in fragment order (losses.pack_conv_weights) and copied linearly; two LDS buffers,
//                                       one barrier per K step, the next step's global loads in flight under the MFMAs.
//   perc_pool / perc_pool_bwd           2 x 2 max pool; the backward finds the arg-max again from the stored activations (first
//                                       maximum in row-major order, torch's tie rule), adds the tap's gradient, applies the ReLU mask
//   perc_tap_loss / perc_tap_features   n = x / (|x|_c + 1e-10) * sqrt(lin_c / (H W)); sum (n_img - n_tgt)^2 and its exact backward
//   perc_reduce                         the loss partials in a fixed order
// No float atomics anywhere: every sum has a fixed order, results are bit-identical from run to run.
#include "ggd_common.h"

#include <algorithm>
#include <utility>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

enum { EPI_FWD = 0, EPI_MASK = 1, EPI_RAW = 2 };

constexpr int PERC_BM = 128;          // pixels per block of perc_conv
constexpr int PERC_TAP_PIX = 16;      // pixels per wave of perc_tap_loss (one loss partial each)
constexpr int LEVEL_OF[GGD_PERC_CONVS] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int TAP_LAYER[GGD_PERC_TAPS] = {1, 3, 6, 9, 12};

__host__ __device__ inline size_t perc_align(size_t n) { return (n + 255) & ~(size_t)255; }

__device__ __forceinline__ float round_split(float v) {   // hi + lo of the split-bf16 pair of v, exact in fp32
  const float hi = (float)(__bf16)v;
  return hi + (float)(__bf16)(v - hi);
}
template <typename T> __device__ __forceinline__ T cvt(float v);
template <> __device__ __forceinline__ _Float16 cvt<_Float16>(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f); }
template <> __device__ __forceinline__ __bf16 cvt<__bf16>(float v) { return (__bf16)v; }
template <> __device__ __forceinline__ float cvt<float>(float v) { return round_split(v); }

template <typename T> __device__ __forceinline__ void load8(const T* p, float* v) {
  if constexpr (sizeof(T) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 a = *reinterpret_cast<const t8*>(p);
    for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
  }
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float* v) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(cvt<T>(v[0]), cvt<T>(v[1]), cvt<T>(v[2]), cvt<T>(v[3]));
    *reinterpret_cast<float4*>(p + 4) = make_float4(cvt<T>(v[4]), cvt<T>(v[5]), cvt<T>(v[6]), cvt<T>(v[7]));
  } else {
    typedef T t8 __attribute__((ext_vector_type(8)));
    t8 a;
    for (int i = 0; i < 8; ++i) a[i] = cvt<T>(v[i]);
    *reinterpret_cast<t8*>(p) = a;
  }
}

// ---- prologue: img [B][3][Hi][Wi] (images b < B) and tgt (images b >= B; may be NULL with n_img == B) -> x0 [n_img H W][3]
__global__ __launch_bounds__(256) void perc_prologue(const float* __restrict__ img, const float* __restrict__ tgt, int B, int n_img,
                                                     int Hi, int Wi, int H, int W, float s0, float s1, float s2, float t0,
                                                     float t1, float t2, float* __restrict__ x0) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= (long)n_img * H * W) return;
  const int x = (int)(m % W), y = (int)((m / W) % H), b = (int)(m / ((long)W * H));
  const int kh = Hi / H, kw = Wi / W;
  const float* src = (b < B ? img + (size_t)b * 3 * Hi * Wi : tgt + (size_t)(b - B) * 3 * Hi * Wi);
  const float sc[3] = {s0, s1, s2}, sh[3] = {t0, t1, t2};
  const float inv = 1.0f / (float)(kh * kw);
  for (int c = 0; c < 3; ++c) {
    float acc = 0.0f;
    for (int i = 0; i < kh; ++i)
      for (int j = 0; j < kw; ++j) acc += src[((size_t)c * Hi + (y * kh + i)) * Wi + (x * kw + j)];
    x0[m * 3 + c] = (acc * inv) * sc[c] + sh[c];
  }
}

// dx0 [B H W][3] -> dimg [B][3][Hi][Wi]
__global__ __launch_bounds__(256) void perc_prologue_bwd(const float* __restrict__ dx0, int B, int Hi, int Wi, int H, int W, float s0,
                                                         float s1, float s2, float* __restrict__ dimg) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * 3 * Hi * Wi) return;
  const int X = (int)(i % Wi), Y = (int)((i / Wi) % Hi), c = (int)((i / ((long)Wi * Hi)) % 3), b = (int)(i / ((long)3 * Wi * Hi));
  const int kh = Hi / H, kw = Wi / W;
  const float sc = c == 0 ? s0 : (c == 1 ? s1 : s2);
  dimg[i] = dx0[(((size_t)b * H + Y / kh) * W + X / kw) * 3 + c] * (sc / (float)(kh * kw));
}

// ---- conv1_1: x0 [M][3] fp32 -> act0 [M][C0]; w0 [27][C0] with k = (ky * 3 + kx) * 3 + ci; bias + ReLU
template <typename TF>
__global__ __launch_bounds__(256) void perc_conv0_fwd(const float* __restrict__ x0, long M, int H, int W, int C0,
                                                      const float* __restrict__ w0, const float* __restrict__ bias,
                                                      TF* __restrict__ out) {
  __shared__ float ws[27 * 64 + 64];
  for (int i = threadIdx.x; i < 27 * C0; i += 256) ws[i] = w0[i];
  for (int i = threadIdx.x; i < C0; i += 256) ws[27 * 64 + i] = bias[i];
  __syncthreads();
  const int G = C0 / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long m = idx / G;
  const int g = (int)(idx % G);
  if (m >= M) return;
  const int x = (int)(m % W), y = (int)((m / W) % H);
  float in[27];
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const bool ok = (unsigned)(y + ky - 1) < (unsigned)H && (unsigned)(x + kx - 1) < (unsigned)W;
      const float* p = x0 + (m + (long)(ky - 1) * W + (kx - 1)) * 3;
      for (int c = 0; c < 3; ++c) in[(ky * 3 + kx) * 3 + c] = ok ? p[c] : 0.0f;
    }
  float acc[8];
  for (int j = 0; j < 8; ++j) acc[j] = ws[27 * 64 + g * 8 + j];
  for (int k = 0; k < 27; ++k)
    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(in[k], ws[k * C0 + g * 8 + j], acc[j]);
  for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.0f);
  store8<TF>(out + m * C0 + g * 8, acc);
}

// backward of conv1_1 to its input: g0 [M][C0] (masked) -> dx0 [M][3]; w0t [9][C0][3] = W[co][ci][ky][kx] at tap ky * 3 + kx,
// read against the pixel at (y - (ky - 1), x - (kx - 1))
template <typename TG>
__global__ __launch_bounds__(256) void perc_conv0_bwd(const TG* __restrict__ g0, long M, int H, int W, int C0,
                                                      const float* __restrict__ w0t, float* __restrict__ dx0) {
  __shared__ float ws[9 * 64 * 3];
  for (int i = threadIdx.x; i < 9 * C0 * 3; i += 256) ws[i] = w0t[i];
  __syncthreads();
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int x = (int)(m % W), y = (int)((m / W) % H);
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      if ((unsigned)(y - ky + 1) >= (unsigned)H || (unsigned)(x - kx + 1) >= (unsigned)W) continue;
      const TG* p = g0 + (m - (long)(ky - 1) * W - (kx - 1)) * C0;
      const float* w = ws + (ky * 3 + kx) * C0 * 3;
      for (int c = 0; c < C0; c += 8) {
        float v[8];
        load8<TG>(p + c, v);
        for (int j = 0; j < 8; ++j) {
          a0 = __builtin_fmaf(v[j], w[(c + j) * 3 + 0], a0);
          a1 = __builtin_fmaf(v[j], w[(c + j) * 3 + 1], a1);
          a2 = __builtin_fmaf(v[j], w[(c + j) * 3 + 2], a2);
        }
      }
    }
  dx0[m * 3 + 0] = a0; dx0[m * 3 + 1] = a1; dx0[m * 3 + 2] = a2;
}

// ---- the implicit-GEMM convolution.  in [M][Cin] (M = images * H * W), wp the packed weights:
//   [K step = tap * (Cin / 32) + chunk][part (hi, lo: split only)][CoutPad / 16 tiles][lane 0..63][8]
// where lane l of tile t holds Wmat[k = 8 (l >> 4) + j][n = 16 t + (l & 15)], k = the channel inside the 32-channel chunk; the tap
// (dy, dx) = (tap / 3 - 1, tap % 3 - 1) reads the pixel at (y + dy, x + dx).  EPI_FWD: out = operand(relu(acc + bias));
// EPI_MASK: out = operand(mask_act > 0 ? acc : 0); EPI_RAW: out = acc (fp32).
template <typename T> struct OperandOf { typedef T type; };
template <> struct OperandOf<float> { typedef __bf16 type; };
template <typename T> struct MaskOf { typedef float type; };          // the forward activation type of the tier T is the gradient type of
template <> struct MaskOf<__bf16> { typedef _Float16 type; };

template <typename V>
__device__ __forceinline__ f4 mfma(const V& a, const V& b, const f4& c) {
  if constexpr (std::is_same<V, h16x8>::value) return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

template <typename T, int CT, int EPI>
__global__ __launch_bounds__(256) void perc_conv(const T* __restrict__ in, long M, int H, int W, int Cin, int Cout, int CoutPad,
                                                 const unsigned char* __restrict__ wp, const float* __restrict__ bias,
                                                 void* __restrict__ out_, const void* __restrict__ mask_) {
  constexpr bool SPLIT = sizeof(T) == 4;
  constexpr int PARTS = SPLIT ? 2 : 1;
  constexpr int BN = CT * 32;
  constexpr int A_BYTES = PERC_BM * 64, B_BYTES = BN * 64;           // one part of one buffer: 32 k x 2 bytes per row / column
  constexpr int BUF_BYTES = PARTS * (A_BYTES + B_BYTES);
  constexpr int BCH = CT / 2;                                        // 16-byte weight pieces per thread and part
  typedef typename OperandOf<T>::type Op;
  typedef Op op8 __attribute__((ext_vector_type(8)));
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
  const long m0 = (long)blockIdx.x * PERC_BM;
  const int n0 = blockIdx.y * BN;
  const int CC = Cin / 32, KT = 9 * CC;

  // the two pixel rows this thread stages: row = (t >> 2) + 64 i, 16-byte piece t & 3
  const int chunk = t & 3;
  long am[2]; int ay[2], ax[2]; bool aok[2]; int a_lds[2];
  for (int i = 0; i < 2; ++i) {
    const int row = (t >> 2) + 64 * i;
    am[i] = m0 + row;
    aok[i] = am[i] < M;
    ax[i] = (int)(am[i] % W); ay[i] = (int)((am[i] / W) % H);
    a_lds[i] = row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4);
  }
  const unsigned char* wblock = wp + (size_t)(n0 / 16) * 1024;
  const size_t w_part = (size_t)(CoutPad / 16) * 1024, w_step = w_part * PARTS;

  float4 areg[2][SPLIT ? 2 : 1];
  uint4 breg[PARTS][BCH];
  auto load_step = [&](int tap, int cc, int ks) {
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    for (int i = 0; i < 2; ++i) {
      const bool ok = aok[i] && (unsigned)(ay[i] + dy) < (unsigned)H && (unsigned)(ax[i] + dx) < (unsigned)W;
      const T* p = in + (am[i] + (long)dy * W + dx) * Cin + cc * 32 + chunk * 8;
      for (int j = 0; j < (SPLIT ? 2 : 1); ++j)
        areg[i][j] = ok ? reinterpret_cast<const float4*>(p)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int part = 0; part < PARTS; ++part)
      for (int j = 0; j < BCH; ++j)
        breg[part][j] = *reinterpret_cast<const uint4*>(wblock + (size_t)ks * w_step + part * w_part + (size_t)(t + 256 * j) * 16);
  };
  auto store_step = [&](unsigned char* buf) {
    for (int i = 0; i < 2; ++i) {
      if constexpr (SPLIT) {
        const float v[8] = {areg[i][0].x, areg[i][0].y, areg[i][0].z, areg[i][0].w, areg[i][1].x, areg[i][1].y, areg[i][1].z, areg[i][1].w};
        bf16x8 hi, lo;
        for (int j = 0; j < 8; ++j) { hi[j] = (__bf16)v[j]; lo[j] = (__bf16)(v[j] - (float)hi[j]); }
        *reinterpret_cast<bf16x8*>(buf + a_lds[i]) = hi;
        *reinterpret_cast<bf16x8*>(buf + A_BYTES + a_lds[i]) = lo;
      } else {
        *reinterpret_cast<float4*>(buf + a_lds[i]) = areg[i][0];
      }
    }
    for (int part = 0; part < PARTS; ++part)
      for (int j = 0; j < BCH; ++j)
        *reinterpret_cast<uint4*>(buf + PARTS * A_BYTES + part * B_BYTES + (t + 256 * j) * 16) = breg[part][j];
  };

  f4 acc[CT][4];
  for (int c = 0; c < CT; ++c)
    for (int p = 0; p < 4; ++p) acc[c][p] = (f4){0.f, 0.f, 0.f, 0.f};

  // fragment addresses: pixel tile p of this wave = rows wm * 64 + 16 p + (lane & 15), k piece lane >> 4
  int xa[4];
  for (int p = 0; p < 4; ++p) {
    const int row = wm * 64 + p * 16 + (lane & 15);
    xa[p] = row * 64 + (((lane >> 4) ^ ((row >> 2) & 3)) << 4);
  }
  const int wa = PARTS * A_BYTES + (wn * CT) * 1024 + lane * 16;

  int tap = 0, cc = 0;
  load_step(0, 0, 0);
  for (int ks = 0; ks < KT; ++ks) {
    unsigned char* buf = lds + (ks & 1) * BUF_BYTES;
    store_step(buf);
    __syncthreads();
    if (++cc == CC) { cc = 0; ++tap; }
    if (ks + 1 < KT) load_step(tap, cc, ks + 1);
    op8 xf[PARTS][4];
    for (int part = 0; part < PARTS; ++part)
      for (int p = 0; p < 4; ++p) xf[part][p] = *reinterpret_cast<const op8*>(buf + part * A_BYTES + xa[p]);
    for (int c = 0; c < CT; ++c) {
      const op8 wh = *reinterpret_cast<const op8*>(buf + wa + c * 1024);
      if constexpr (SPLIT) {
        const op8 wl = *reinterpret_cast<const op8*>(buf + wa + B_BYTES + c * 1024);
        for (int p = 0; p < 4; ++p) {
          acc[c][p] = mfma<op8>(wl, xf[0][p], acc[c][p]);
          acc[c][p] = mfma<op8>(wh, xf[1][p], acc[c][p]);
          acc[c][p] = mfma<op8>(wh, xf[0][p], acc[c][p]);
        }
      } else {
        for (int p = 0; p < 4; ++p) acc[c][p] = mfma<op8>(wh, xf[0][p], acc[c][p]);
      }
    }
  }

  // epilogue: lane holds channels n0 + 16 (wn CT + c) + 4 (lane >> 4) + r of pixel m0 + wm * 64 + 16 p + (lane & 15)
  for (int p = 0; p < 4; ++p) {
    const long m = m0 + wm * 64 + p * 16 + (lane & 15);
    if (m >= M) continue;
    for (int c = 0; c < CT; ++c) {
      const int n = n0 + (wn * CT + c) * 16 + (lane >> 4) * 4;
      if (n >= Cout) continue;
      const size_t o = (size_t)m * Cout + n;
      f4 v = acc[c][p];
      if constexpr (EPI == EPI_RAW) {
        *reinterpret_cast<float4*>(static_cast<float*>(out_) + o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        if constexpr (EPI == EPI_FWD) {
          const float4 b = *reinterpret_cast<const float4*>(bias + n);
          v[0] = fmaxf(v[0] + b.x, 0.f); v[1] = fmaxf(v[1] + b.y, 0.f); v[2] = fmaxf(v[2] + b.z, 0.f); v[3] = fmaxf(v[3] + b.w, 0.f);
        } else {
          typedef typename MaskOf<T>::type TM;
          const TM* a = static_cast<const TM*>(mask_) + o;
          for (int r = 0; r < 4; ++r) v[r] = (float)a[r] > 0.f ? v[r] : 0.f;
        }
        T* dst = static_cast<T*>(out_) + o;
        if constexpr (SPLIT) {
          *reinterpret_cast<float4*>(dst) = make_float4(round_split(v[0]), round_split(v[1]), round_split(v[2]), round_split(v[3]));
        } else {
          typedef T t4 __attribute__((ext_vector_type(4)));
          t4 r4;
          for (int r = 0; r < 4; ++r) r4[r] = cvt<T>(v[r]);
          *reinterpret_cast<t4*>(dst) = r4;
        }
      }
    }
  }
}

// ---- 2 x 2 max pool: in [n_img H W][C] -> out [n_img H/2 W/2][C]; one thread per (output pixel, 8 channels)
template <typename T>
__global__ __launch_bounds__(256) void perc_pool(const T* __restrict__ in, long Mo, int Ho, int Wo, int C, T* __restrict__ out) {
  const int G = C / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long mo = idx / G;
  const int g = (int)(idx % G);
  if (mo >= Mo) return;
  const int x = (int)(mo % Wo), y = (int)((mo / Wo) % Ho);
  const long b = mo / ((long)Wo * Ho);
  const long base = ((b * 2 * Ho + 2 * y) * 2 * Wo + 2 * x);
  float best[8], v[8];
  load8<T>(in + base * C + g * 8, best);
  const long offs[3] = {1, 2L * Wo, 2L * Wo + 1};
  for (int k = 0; k < 3; ++k) {
    load8<T>(in + (base + offs[k]) * C + g * 8, v);
    for (int j = 0; j < 8; ++j) best[j] = v[j] > best[j] ? v[j] : best[j];
  }
  store8<T>(out + mo * C + g * 8, best);   // the values are operand-exact already: the conversion changes nothing
}

// backward of [ReLU, tap, pool]: act [.. H W][C] (the first Mo * 4 pixels = the image half), draw [Mo][C] fp32 the gradient at
// the pooled map, tapgrad [Mo * 4][C] fp32 the tap's gradient at act -> g [Mo * 4][C] = operand((act > 0) * (routed + tap))
template <typename TF, typename TG>
__global__ __launch_bounds__(256) void perc_pool_bwd(const TF* __restrict__ act, const float* __restrict__ draw,
                                                     const float* __restrict__ tapgrad, long Mo, int Ho, int Wo, int C,
                                                     TG* __restrict__ g) {
  const int G = C / 8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long mo = idx / G;
  const int gch = (int)(idx % G);
  if (mo >= Mo) return;
  const int x = (int)(mo % Wo), y = (int)((mo / Wo) % Ho);
  const long b = mo / ((long)Wo * Ho);
  const long base = ((b * 2 * Ho + 2 * y) * 2 * Wo + 2 * x);
  const long offs[4] = {0, 1, 2L * Wo, 2L * Wo + 1};
  float a[4][8], d[8];
  for (int k = 0; k < 4; ++k) load8<TF>(act + (base + offs[k]) * C + gch * 8, a[k]);
  load8<float>(draw + mo * C + gch * 8, d);
  int arg[8];
  for (int j = 0; j < 8; ++j) {
    float best = a[0][j];
    arg[j] = 0;
    for (int k = 1; k < 4; ++k)
      if (a[k][j] > best) { best = a[k][j]; arg[j] = k; }   // strictly greater: the first maximum in row-major order keeps it
  }
  for (int k = 0; k < 4; ++k) {
    float tg[8], o[8];
    load8<float>(tapgrad + (base + offs[k]) * C + gch * 8, tg);
    for (int j = 0; j < 8; ++j) o[j] = a[k][j] > 0.f ? (arg[j] == k ? d[j] : 0.f) + tg[j] : 0.f;
    store8<TG>(g + (base + offs[k]) * C + gch * 8, o);
  }
}

// ---- taps
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// act [2 B HW][C]: image pixels first, target pixels B * HW later.  One wave per PERC_TAP_PIX consecutive image pixels, lane l holds
// channels l + 64 i.  partials[wave] = the wave's share of sum (n_img - n_tgt)^2; grad (may be NULL) [B HW][C] = (act > 0) * dloss/dact,
// fp32, or in the gradient operand format when LAST (conv5_3's tap: nothing is added to it).
template <typename TF, typename TG, bool LAST>
__global__ __launch_bounds__(256) void perc_tap_loss(const TF* __restrict__ act, long Mi, int HW, int C, const float* __restrict__ lin,
                                                     float* __restrict__ partials, void* __restrict__ grad_) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long first = wave * PERC_TAP_PIX;
  if (first >= Mi) return;
  const int NI = (C + 63) / 64;
  float w[8];
  for (int i = 0; i < 8; ++i) w[i] = (i < NI && lane + 64 * i < C) ? sqrtf(lin[lane + 64 * i] / (float)HW) : 0.f;
  float total = 0.f;
  for (long m = first; m < first + PERC_TAP_PIX && m < Mi; ++m) {
    float a[8], tv[8], sa = 0.f, st = 0.f;
    for (int i = 0; i < 8; ++i) {
      const bool on = i < NI && lane + 64 * i < C;
      a[i] = on ? (float)act[m * C + lane + 64 * i] : 0.f;
      tv[i] = on ? (float)act[(Mi + m) * C + lane + 64 * i] : 0.f;
      sa = __builtin_fmaf(a[i], a[i], sa);
      st = __builtin_fmaf(tv[i], tv[i], st);
    }
    const float na = sqrtf(wave_sum(sa)), nt = sqrtf(wave_sum(st));
    const float ia = 1.0f / (na + 1e-10f), it = 1.0f / (nt + 1e-10f);
    float u[8], sq = 0.f, dot = 0.f;
    for (int i = 0; i < 8; ++i) {
      const float d = w[i] * (a[i] * ia - tv[i] * it);
      sq = __builtin_fmaf(d, d, sq);
      u[i] = 2.0f * w[i] * d;
      dot = __builtin_fmaf(u[i], a[i], dot);
    }
    total += wave_sum(sq);
    if (grad_) {
      // d/da_j = u_j / (|a| + eps) - (a_j / |a|) sum_c(u_c a_c) / (|a| + eps)^2; a pixel whose channels are all zero keeps the first term
      const float s = na > 0.f ? wave_sum(dot) * ia * ia / na : 0.f;
      for (int i = 0; i < NI; ++i) {
        const int c = lane + 64 * i;
        if (c >= C) continue;
        const float gv = a[i] > 0.f ? u[i] * ia - a[i] * s : 0.f;
        if constexpr (LAST) static_cast<TG*>(grad_)[m * C + c] = cvt<TG>(gv);
        else static_cast<float*>(grad_)[m * C + c] = gv;
      }
    }
  }
  if (lane == 0) partials[wave] = total;
}

// feat[b][off + c * HW + p] = n_c * sqrt(lin_c / HW): the rows of PerceptualStandIn.features.  One wave per pixel.
template <typename TF>
__global__ __launch_bounds__(256) void perc_tap_features(const TF* __restrict__ act, long Mt, int HW, int C, const float* __restrict__ lin,
                                                         float* __restrict__ feat, long F, long off) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= Mt) return;
  const int NI = (C + 63) / 64;
  float a[8], sa = 0.f;
  for (int i = 0; i < 8; ++i) {
    a[i] = (i < NI && lane + 64 * i < C) ? (float)act[m * C + lane + 64 * i] : 0.f;
    sa = __builtin_fmaf(a[i], a[i], sa);
  }
  const float ia = 1.0f / (sqrtf(wave_sum(sa)) + 1e-10f);
  const long b = m / HW, p = m % HW;
  for (int i = 0; i < NI; ++i) {
    const int c = lane + 64 * i;
    if (c < C) feat[b * F + off + (long)c * HW + p] = a[i] * ia * sqrtf(lin[c] / (float)HW);
  }
}

__global__ __launch_bounds__(256) void perc_reduce(const float* __restrict__ partials, long n, float* __restrict__ out) {
  __shared__ float s[256];
  float acc = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) acc += partials[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s[0];
}

// ---- host side
struct PercLayout {
  int Hl[5], Wl[5];
  size_t x0, act[GGD_PERC_CONVS], pooled[4], ga, gb, draw, tapgrad, dx0, partials, total;
  long n_partials[GGD_PERC_TAPS], partial_off[GGD_PERC_TAPS], partial_count;
};

bool perc_shape_ok(const ggd_perceptual_desc* d) {
  if (!d || (d->tier != GGD_PERC_BF16 && d->tier != GGD_PERC_FP32) || d->B <= 0 || d->H <= 0 || d->W <= 0) return false;
  if (d->H % 16 || d->W % 16 || d->H_in <= 0 || d->W_in <= 0 || d->H_in % d->H || d->W_in % d->W) return false;
  for (int l = 0; l < GGD_PERC_CONVS; ++l)
    if (d->widths[l] <= 0 || d->widths[l] % 32 || d->widths[l] > 512) return false;
  if (d->widths[0] > 64) return false;
  return true;
}

PercLayout perc_layout(const ggd_perceptual_desc* d, int n_img, bool with_grad) {
  PercLayout L{};
  const size_t ef = d->tier == GGD_PERC_FP32 ? 4 : 2;
  for (int r = 0; r < 5; ++r) { L.Hl[r] = d->H >> r; L.Wl[r] = d->W >> r; }
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += perc_align(bytes); return at; };
  L.x0 = take((size_t)n_img * d->H * d->W * 3 * 4);
  for (int l = 0; l < GGD_PERC_CONVS; ++l) {
    const int r = LEVEL_OF[l];
    L.act[l] = take((size_t)n_img * L.Hl[r] * L.Wl[r] * d->widths[l] * ef);
  }
  for (int k = 0; k < 4; ++k) L.pooled[k] = take((size_t)n_img * L.Hl[k + 1] * L.Wl[k + 1] * d->widths[TAP_LAYER[k]] * ef);
  long np = 0;
  for (int k = 0; k < GGD_PERC_TAPS; ++k) {
    const long mi = (long)d->B * L.Hl[k] * L.Wl[k];
    L.n_partials[k] = (mi + PERC_TAP_PIX - 1) / PERC_TAP_PIX;
    L.partial_off[k] = np;
    np += L.n_partials[k];
  }
  L.partial_count = np;
  L.partials = take((size_t)np * 4);
  if (with_grad) {
    size_t gmax = 0, dmax = 0, tmax = 0;
    for (int l = 0; l < GGD_PERC_CONVS; ++l) {
      const int r = LEVEL_OF[l];
      gmax = std::max(gmax, (size_t)d->B * L.Hl[r] * L.Wl[r] * d->widths[l] * ef);
    }
    for (int k = 0; k < 4; ++k) {
      dmax = std::max(dmax, (size_t)d->B * L.Hl[k + 1] * L.Wl[k + 1] * d->widths[TAP_LAYER[k]] * 4);
      tmax = std::max(tmax, (size_t)d->B * L.Hl[k] * L.Wl[k] * d->widths[TAP_LAYER[k]] * 4);
    }
    L.ga = take(gmax); L.gb = take(gmax); L.draw = take(dmax); L.tapgrad = take(tmax);
    L.dx0 = take((size_t)d->B * d->H * d->W * 3 * 4);
  }
  L.total = o;
  return L;
}

inline unsigned blocks_for(long n, int per) { return (unsigned)((n + per - 1) / per); }

template <typename T, int EPI>
void launch_conv(hipStream_t s, const T* in, long M, int H, int W, int Cin, int Cout, const void* wp, const float* bias, void* out,
                 const void* mask) {
  const unsigned char* w = static_cast<const unsigned char*>(wp);
  if (Cout % 128 == 0) {
    hipLaunchKernelGGL((perc_conv<T, 4, EPI>), dim3(blocks_for(M, PERC_BM), Cout / 128), dim3(256), 0, s, in, M, H, W, Cin, Cout,
                       Cout, w, bias, out, mask);
  } else {
    const int pad = (Cout + 63) / 64 * 64;
    hipLaunchKernelGGL((perc_conv<T, 2, EPI>), dim3(blocks_for(M, PERC_BM), pad / 64), dim3(256), 0, s, in, M, H, W, Cin, Cout, pad,
                       w, bias, out, mask);
  }
}

// forward of n_img images (image batch first, then the target batch) up to the last activation
template <typename TF>
void perc_forward(hipStream_t s, const ggd_perceptual_desc* d, const PercLayout& L, unsigned char* tmp, const float* img,
                  const float* tgt, int n_img) {
  const long M0 = (long)n_img * d->H * d->W;
  float* x0 = reinterpret_cast<float*>(tmp + L.x0);
  hipLaunchKernelGGL(perc_prologue, dim3(blocks_for(M0, 256)), dim3(256), 0, s, img, tgt, d->B, n_img, d->H_in, d->W_in, d->H, d->W,
                     d->scale[0], d->scale[1], d->scale[2], d->shift[0], d->shift[1], d->shift[2], x0);
  const int C0 = d->widths[0];
  hipLaunchKernelGGL((perc_conv0_fwd<TF>), dim3(blocks_for(M0 * (C0 / 8), 256)), dim3(256), 0, s, x0, M0, d->H, d->W, C0, d->w0,
                     d->bias[0], reinterpret_cast<TF*>(tmp + L.act[0]));
  for (int l = 1; l < GGD_PERC_CONVS; ++l) {
    const int r = LEVEL_OF[l];
    const long M = (long)n_img * L.Hl[r] * L.Wl[r];
    const TF* in = reinterpret_cast<const TF*>(tmp + L.act[l - 1]);
    if (LEVEL_OF[l - 1] != r) {
      TF* pooled = reinterpret_cast<TF*>(tmp + L.pooled[r - 1]);
      hipLaunchKernelGGL((perc_pool<TF>), dim3(blocks_for(M * (d->widths[l - 1] / 8), 256)), dim3(256), 0, s, in, M, L.Hl[r], L.Wl[r],
                         d->widths[l - 1], pooled);
      in = pooled;
    }
    launch_conv<TF, EPI_FWD>(s, in, M, L.Hl[r], L.Wl[r], d->widths[l - 1], d->widths[l], d->w_fwd[l], d->bias[l], tmp + L.act[l],
                             nullptr);
  }
}

template <typename TF, typename TG>
void perc_loss_impl(hipStream_t s, const ggd_perceptual_desc* d, const PercLayout& L, unsigned char* tmp, const float* img,
                    const float* tgt, float* loss, float* grad) {
  perc_forward<TF>(s, d, L, tmp, img, tgt, 2 * d->B);
  float* partials = reinterpret_cast<float*>(tmp + L.partials);
  auto tap = [&](int k, void* gout) {
    const int l = TAP_LAYER[k];
    const long Mi = (long)d->B * L.Hl[k] * L.Wl[k];
    const dim3 grid(blocks_for(L.n_partials[k], 4));
    const TF* act = reinterpret_cast<const TF*>(tmp + L.act[l]);
    if (k == GGD_PERC_TAPS - 1)
      hipLaunchKernelGGL((perc_tap_loss<TF, TG, true>), grid, dim3(256), 0, s, act, Mi, L.Hl[k] * L.Wl[k], d->widths[l], d->lin[k],
                         partials + L.partial_off[k], gout);
    else
      hipLaunchKernelGGL((perc_tap_loss<TF, TG, false>), grid, dim3(256), 0, s, act, Mi, L.Hl[k] * L.Wl[k], d->widths[l], d->lin[k],
                         partials + L.partial_off[k], gout);
  };
  if (!grad) {
    for (int k = 0; k < GGD_PERC_TAPS; ++k) tap(k, nullptr);
  } else {
    unsigned char *ga = tmp + L.ga, *gb = tmp + L.gb;
    float* draw = reinterpret_cast<float*>(tmp + L.draw);
    float* tapgrad = reinterpret_cast<float*>(tmp + L.tapgrad);
    tap(GGD_PERC_TAPS - 1, ga);                                   // g[12]
    for (int l = GGD_PERC_CONVS - 1; l >= 1; --l) {               // g[l] in ga -> g[l - 1] in gb
      const int r = LEVEL_OF[l];
      const long M = (long)d->B * L.Hl[r] * L.Wl[r];
      const int Cg = d->widths[l], Cx = d->widths[l - 1];
      if (LEVEL_OF[l - 1] != r) {
        launch_conv<TG, EPI_RAW>(s, reinterpret_cast<const TG*>(ga), M, L.Hl[r], L.Wl[r], Cg, Cx, d->w_bwd[l], nullptr, draw, nullptr);
        tap(r - 1, tapgrad);
        hipLaunchKernelGGL((perc_pool_bwd<TF, TG>), dim3(blocks_for(M * (Cx / 8), 256)), dim3(256), 0, s,
                           reinterpret_cast<const TF*>(tmp + L.act[l - 1]), draw, tapgrad, M, L.Hl[r], L.Wl[r], Cx,
                           reinterpret_cast<TG*>(gb));
      } else {
        launch_conv<TG, EPI_MASK>(s, reinterpret_cast<const TG*>(ga), M, L.Hl[r], L.Wl[r], Cg, Cx, d->w_bwd[l], nullptr, gb,
                                  tmp + L.act[l - 1]);
      }
      std::swap(ga, gb);
    }
    const long M0 = (long)d->B * d->H * d->W;
    float* dx0 = reinterpret_cast<float*>(tmp + L.dx0);
    hipLaunchKernelGGL((perc_conv0_bwd<TG>), dim3(blocks_for(M0, 256)), dim3(256), 0, s, reinterpret_cast<const TG*>(ga), M0, d->H, d->W,
                       d->widths[0], d->w0_t, dx0);
    hipLaunchKernelGGL(perc_prologue_bwd, dim3(blocks_for((long)d->B * 3 * d->H_in * d->W_in, 256)), dim3(256), 0, s, dx0, d->B, d->H_in,
                       d->W_in, d->H, d->W, d->scale[0], d->scale[1], d->scale[2], grad);
  }
  hipLaunchKernelGGL(perc_reduce, dim3(1), dim3(256), 0, s, partials, L.partial_count, loss);
}

template <typename TF>
void perc_features_impl(hipStream_t s, const ggd_perceptual_desc* d, const PercLayout& L, unsigned char* tmp, const float* img, float* feat) {
  perc_forward<TF>(s, d, L, tmp, img, nullptr, d->B);
  long F = 0, off[GGD_PERC_TAPS];
  for (int k = 0; k < GGD_PERC_TAPS; ++k) { off[k] = F; F += (long)d->widths[TAP_LAYER[k]] * L.Hl[k] * L.Wl[k]; }
  for (int k = 0; k < GGD_PERC_TAPS; ++k) {
    const long Mt = (long)d->B * L.Hl[k] * L.Wl[k];
    hipLaunchKernelGGL((perc_tap_features<TF>), dim3(blocks_for(Mt, 4)), dim3(256), 0, s,
                       reinterpret_cast<const TF*>(tmp + L.act[TAP_LAYER[k]]), Mt, L.Hl[k] * L.Wl[k], d->widths[TAP_LAYER[k]], d->lin[k],
                       feat, F, off[k]);
  }
}

bool perc_pointers_ok(const ggd_perceptual_desc* d, bool with_grad) {
  if (!d->w0 || (with_grad && !d->w0_t)) return false;
  for (int l = 0; l < GGD_PERC_CONVS; ++l)
    if (!d->bias[l] || (l > 0 && (!d->w_fwd[l] || (with_grad && !d->w_bwd[l])))) return false;
  for (int k = 0; k < GGD_PERC_TAPS; ++k)
    if (!d->lin[k]) return false;
  return true;
}

}  // namespace

extern "C" size_t ggd_perceptual_tmp_bytes(const ggd_perceptual_desc* desc, int32_t n_images, int32_t with_grad) {
  if (!perc_shape_ok(desc) || n_images <= 0) return 0;
  return perc_layout(desc, n_images, with_grad != 0).total;
}

extern "C" int ggd_perceptual_loss(ggd_ctx* ctx, void* stream, const ggd_perceptual_desc* desc, const float* image, const float* target,
                                   float* loss, float* grad_image, void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (!perc_shape_ok(desc)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_perceptual_loss: unsupported shape, width or tier");
  if (!image || !target || !loss || !tmp || !perc_pointers_ok(desc, grad_image != nullptr))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_perceptual_loss: NULL pointer");
  const PercLayout L = perc_layout(desc, 2 * desc->B, grad_image != nullptr);
  if (tmp_bytes < L.total) return ggd_fail(ctx, GGD_E_INVALID, "ggd_perceptual_loss: tmp too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* t = static_cast<unsigned char*>(tmp);
  if (desc->tier == GGD_PERC_BF16) perc_loss_impl<_Float16, __bf16>(s, desc, L, t, image, target, loss, grad_image);
  else perc_loss_impl<float, float>(s, desc, L, t, image, target, loss, grad_image);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_perceptual_features(ggd_ctx* ctx, void* stream, const ggd_perceptual_desc* desc, const float* image, float* features,
                                       void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (!perc_shape_ok(desc)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_perceptual_features: unsupported shape, width or tier");
  if (!image || !features || !tmp || !perc_pointers_ok(desc, false))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_perceptual_features: NULL pointer");
  const PercLayout L = perc_layout(desc, desc->B, false);
  if (tmp_bytes < L.total) return ggd_fail(ctx, GGD_E_INVALID, "ggd_perceptual_features: tmp too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* t = static_cast<unsigned char*>(tmp);
  if (desc->tier == GGD_PERC_BF16) perc_features_impl<_Float16>(s, desc, L, t, image, features);
  else perc_features_impl<float>(s, desc, L, t, image, features);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
