// ggd_imgloss.hip -- fused image losses of the decoder training step.
//
// Replaces, for one rendered image [3,H,W] against its target, the PyTorch graph of
//   l1_loss / l2_loss / ssim   gaussian_splatting/utils/loss_utils.py:17-63  (11x11 Gaussian window, sigma 1.5, zero
//                              padding, C1 = 0.01^2, C2 = 0.03^2, mean over 3*H*W)
//   sobel_loss                 main/loss_utils/sobel_loss.py:19-30            (3x3 Sobel x / y cross-correlation SUMMED
//                              over the three channels, squared difference, mean over H*W)
// as used in main/train_pano2gaussian_decoder.py:246-261:
//   loss = w_l1 * L1 + w_l2 * L2 + w_ssim * (1 - SSIM) + w_sobel * Sobel
// -- about 60 small kernels forward + backward in PyTorch -- by three launches that produce the four loss terms AND
// dloss/dimage in one go (the loss is a scalar with known weights, so its gradient is formed directly):
//   A  ssim_stats_kernel  per 32x32 tile and channel: separable 11-tap blur of x, y, x^2, y^2, xy through LDS, the SSIM
//                         map, its partial derivatives w.r.t. the blurred moments (maps a, b, c), block-reduced sums of
//                         SSIM, |x-y|, (x-y)^2
//   B  sobel_kernel       channel-summed difference image -> Sobel responses gx, gy (maps) and the sum of gx^2 + gy^2
//   C  grad_kernel        dL/dx = -w_ssim/(3HW) [G*a + 2x G*b + y G*c] + L1 / L2 terms + the transposed Sobel stencil on
//                         (gx, gy); thread 0 also finalises the loss terms.
// All stencil work is HBM-trivial (a 512x512 image is 3 MB); what matters is the launch count on the step's critical
// path.  SSIM algebra: S = A1 A2 / (B1 B2), A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1,
// B2 = s11 + s22 + C2 with s11 = G*x^2 - mu1^2, s12 = G*xy - mu1 mu2;  c = dS/ds12 = 2 A1/(B1 B2),
// b = dS/ds11 = -S/B2,  a = dS/dmu1 (total) = 2 mu2 A2/(B1 B2) - 2 mu1 S/B1 - 2 mu1 b - mu2 c.
//
// MASKED instances (ggd_image_loss_masked; --apply_mask_to_rendering, main/train_pano2gaussian_decoder.py:237-241): the
// generator's low-resolution mask [mask_h, mask_w] is upsampled bilinearly by the integer factors H / mask_h, W / mask_w
// (PyTorch's interpolate, align_corners=False) and image and target are composited onto white, x' = (x*m + 1) - m, at the
// place where each of the three kernels reads a pixel INSIDE the image -- no full-resolution mask, no composited image, no
// extra launch, the same tmp layout.  Pixels outside the image stay 0 (the reference zero-pads the composited image).
// grad_kernel forms the gradient from x', y' and applies the chain rule dL/dx = m dL/dx' before the store; target and mask
// get no gradient (the reference's mask comes out of a no_grad synthesis).  The <false> instances are the unmasked code.
// mask_composite_kernel is the same composite as an operator of its own (forward x', backward g*m) for the consumers that
// need the composited image itself (the perceptual term, logging, eval).
#include "ggd_common.h"

namespace {

constexpr int TILE = 32;
constexpr int HALO = 5;
constexpr int EXT = TILE + 2 * HALO;  // 42

struct Win { float g[11]; };

// The low-resolution mask and the upsample factors; m == nullptr in the unmasked instances (never read there).
struct Mask { const float* m; int w, h; float fx, fy; };

// One axis of PyTorch's bilinear upsample with align_corners=False: the two source cells and the weight of the second.
struct MaskAxis { int i0, i1; float l; };

__device__ __forceinline__ MaskAxis mask_axis(int dst, float f, int n) {
  const float src = fmaxf(((float)dst + 0.5f) / f - 0.5f, 0.f);
  MaskAxis a;
  a.i0 = min((int)src, n - 1);
  a.i1 = min(a.i0 + 1, n - 1);
  a.l = src - (float)a.i0;
  return a;
}

// along x for both rows, then along y; a factor of 1 gives l = 0 and returns the cell unchanged
__device__ __forceinline__ float mask_blend(float v00, float v01, float v10, float v11, const MaskAxis& ay, const MaskAxis& ax) {
  const float top = v00 * (1.f - ax.l) + v01 * ax.l;
  const float bot = v10 * (1.f - ax.l) + v11 * ax.l;
  return top * (1.f - ay.l) + bot * ay.l;
}

__device__ __forceinline__ float mask_value(const Mask& mk, const MaskAxis& ay, const MaskAxis& ax) {
  const float* r0 = mk.m + (size_t)ay.i0 * mk.w;
  const float* r1 = mk.m + (size_t)ay.i1 * mk.w;
  return mask_blend(r0[ax.i0], r0[ax.i1], r1[ax.i0], r1[ax.i1], ay, ax);
}

__device__ __forceinline__ float mask_at(const Mask& mk, int gy, int gx) {
  return mask_value(mk, mask_axis(gy, mk.fy, mk.h), mask_axis(gx, mk.fx, mk.w));
}

// onto white, in the reference's order (image * m + 1 - m)
__device__ __forceinline__ float composite(float v, float m) { return (v * m + 1.f) - m; }

__device__ __forceinline__ float block_sum(float v, float* red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float s = 0.f;
  if (tid == 0) s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

template <bool MASKED>
__global__ __launch_bounds__(256) void ssim_stats_kernel(int W, int H, Win win, const float* __restrict__ img,
                                                         const float* __restrict__ tgt, float* __restrict__ abc,
                                                         float* __restrict__ sums, Mask mk) {
  __shared__ float sx[EXT][EXT + 1], sy[EXT][EXT + 1];
  __shared__ float hb[5][EXT][TILE + 1];
  __shared__ float red[4];
  const int tid = threadIdx.x, ch = blockIdx.z;
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  const size_t plane = (size_t)H * W;
  const float* X = img + ch * plane;
  const float* Y = tgt + ch * plane;
  for (int i = tid; i < EXT * EXT; i += 256) {
    const int r = i / EXT, c = i % EXT;
    const int gy = y0 + r - HALO, gx = x0 + c - HALO;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    if constexpr (MASKED) {   // halo pixels outside the image stay 0, not 1 - m
      float a = 0.f, b = 0.f;
      if (in) {
        const float m = mask_at(mk, gy, gx);
        a = composite(X[(size_t)gy * W + gx], m);
        b = composite(Y[(size_t)gy * W + gx], m);
      }
      sx[r][c] = a; sy[r][c] = b;
    } else {
      sx[r][c] = in ? X[(size_t)gy * W + gx] : 0.f;
      sy[r][c] = in ? Y[(size_t)gy * W + gx] : 0.f;
    }
  }
  __syncthreads();
  for (int i = tid; i < EXT * TILE; i += 256) {
    const int r = i / TILE, c = i % TILE;
    float m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float a = sx[r][c + k], b = sy[r][c + k], g = win.g[k];
      m1 += g * a; m2 += g * b; e11 += g * (a * a); e22 += g * (b * b); e12 += g * (a * b);
    }
    hb[0][r][c] = m1; hb[1][r][c] = m2; hb[2][r][c] = e11; hb[3][r][c] = e22; hb[4][r][c] = e12;
  }
  __syncthreads();
  const int tx = tid & 31, ty = tid >> 5;
  float s_ssim = 0, s_l1 = 0, s_l2 = 0;
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    const int gy = y0 + r, gx = x0 + tx;
    if (gy >= H || gx >= W) continue;
    float m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float g = win.g[k];
      m1 += g * hb[0][r + k][tx]; m2 += g * hb[1][r + k][tx]; e11 += g * hb[2][r + k][tx];
      e22 += g * hb[3][r + k][tx]; e12 += g * hb[4][r + k][tx];
    }
    const float s11 = e11 - m1 * m1, s22 = e22 - m2 * m2, s12 = e12 - m1 * m2;
    const float A1 = 2.f * m1 * m2 + C1, A2 = 2.f * s12 + C2, B1 = m1 * m1 + m2 * m2 + C1, B2 = s11 + s22 + C2;
    const float inv = 1.0f / (B1 * B2);
    const float S = A1 * A2 * inv;
    const float c = 2.f * A1 * inv;
    const float b = -S / B2;
    const float a = 2.f * m2 * A2 * inv - 2.f * m1 * S / B1 - 2.f * m1 * b - m2 * c;
    const size_t p = (size_t)gy * W + gx;
    abc[(ch * 3 + 0) * plane + p] = a;
    abc[(ch * 3 + 1) * plane + p] = b;
    abc[(ch * 3 + 2) * plane + p] = c;
    const float d = sx[r + HALO][tx + HALO] - sy[r + HALO][tx + HALO];
    s_ssim += S; s_l1 += fabsf(d); s_l2 += d * d;
  }
  const float t0 = block_sum(s_ssim, red), t1 = block_sum(s_l1, red), t2 = block_sum(s_l2, red);
  if (tid == 0) { atomicAdd(sums + 0, t1); atomicAdd(sums + 1, t2); atomicAdd(sums + 2, t0); }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void sobel_kernel(int W, int H, const float* __restrict__ img,
                                                    const float* __restrict__ tgt, float* __restrict__ gxy,
                                                    float* __restrict__ sums, Mask mk) {
  __shared__ float red[4];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const size_t plane = (size_t)H * W;
  float v = 0.f;
  if (x < W && y < H) {
    float d[3][3];
    [[maybe_unused]] MaskAxis ay[3], ax[3];   // the upsample is separable: three rows and three columns serve the nine stencil pixels
    if constexpr (MASKED) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {   // (clamped: the axes of pixels outside the image are never used)
        ay[u] = mask_axis(min(max(y + u - 1, 0), H - 1), mk.fy, mk.h);
        ax[u] = mask_axis(min(max(x + u - 1, 0), W - 1), mk.fx, mk.w);
      }
    }
#pragma unroll
    for (int u = -1; u <= 1; ++u)
#pragma unroll
      for (int w = -1; w <= 1; ++w) {
        const int yy = y + u, xx = x + w;
        float s = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
          const size_t p = (size_t)yy * W + xx;
          if constexpr (MASKED) {
            const float m = mask_value(mk, ay[u + 1], ax[w + 1]);
            s = (composite(img[p], m) - composite(tgt[p], m)) +
                (composite(img[plane + p], m) - composite(tgt[plane + p], m)) +
                (composite(img[2 * plane + p], m) - composite(tgt[2 * plane + p], m));
          } else {
            s = (img[p] - tgt[p]) + (img[plane + p] - tgt[plane + p]) + (img[2 * plane + p] - tgt[2 * plane + p]);
          }
        }
        d[u + 1][w + 1] = s;
      }
    // sobel_x = [[1,0,-1],[2,0,-2],[1,0,-1]], sobel_y = [[1,2,1],[0,0,0],[-1,-2,-1]] (cross-correlation)
    const float gx = (d[0][0] - d[0][2]) + 2.f * (d[1][0] - d[1][2]) + (d[2][0] - d[2][2]);
    const float gy = (d[0][0] + 2.f * d[0][1] + d[0][2]) - (d[2][0] + 2.f * d[2][1] + d[2][2]);
    const size_t p = (size_t)y * W + x;
    gxy[p] = gx; gxy[plane + p] = gy;
    v = gx * gx + gy * gy;
  }
  const float t = block_sum(v, red);
  if (threadIdx.x == 0) atomicAdd(sums + 3, t);
}

template <bool MASKED>
__global__ __launch_bounds__(256) void grad_kernel(int W, int H, Win win, const float* __restrict__ img,
                                                   const float* __restrict__ tgt, const float* __restrict__ abc,
                                                   const float* __restrict__ gxy, const float* __restrict__ sums,
                                                   float w_l1, float w_l2, float w_ssim, float w_sobel,
                                                   float* __restrict__ grad, float* __restrict__ terms, Mask mk) {
  __shared__ float sm[3][EXT][EXT + 1];
  __shared__ float hb[3][EXT][TILE + 1];
  const int tid = threadIdx.x, ch = blockIdx.z;
  const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
  const size_t plane = (size_t)H * W;
  const float n3 = 3.0f * (float)H * (float)W, n1 = (float)H * (float)W;
  if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 && ch == 0) {
    const float l1 = sums[0] / n3, l2 = sums[1] / n3, ds = 1.0f - sums[2] / n3, sb = sums[3] / n1;
    terms[0] = l1; terms[1] = l2; terms[2] = ds; terms[3] = sb;
    terms[4] = w_l1 * l1 + w_l2 * l2 + w_ssim * ds + w_sobel * sb;
  }
  for (int i = tid; i < EXT * EXT; i += 256) {
    const int r = i / EXT, c = i % EXT;
    const int gy = y0 + r - HALO, gx = x0 + c - HALO;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const size_t p = in ? (size_t)gy * W + gx : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) sm[k][r][c] = in ? abc[(ch * 3 + k) * plane + p] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < EXT * TILE; i += 256) {
    const int r = i / TILE, c = i % TILE;
    float s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float g = win.g[k];
      s0 += g * sm[0][r][c + k]; s1 += g * sm[1][r][c + k]; s2 += g * sm[2][r][c + k];
    }
    hb[0][r][c] = s0; hb[1][r][c] = s1; hb[2][r][c] = s2;
  }
  __syncthreads();
  const int tx = tid & 31, ty = tid >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    const int gy = y0 + r, gx = x0 + tx;
    if (gy >= H || gx >= W) continue;
    float Ga = 0, Gb = 0, Gc = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float g = win.g[k];
      Ga += g * hb[0][r + k][tx]; Gb += g * hb[1][r + k][tx]; Gc += g * hb[2][r + k][tx];
    }
    const size_t p = (size_t)gy * W + gx;
    float x = img[ch * plane + p], y = tgt[ch * plane + p];
    [[maybe_unused]] float m = 1.f;
    if constexpr (MASKED) {   // everything below is d loss / d x' of the composited pair
      m = mask_at(mk, gy, gx);
      x = composite(x, m); y = composite(y, m);
    }
    const float d = x - y;
    float gsum = -w_ssim / n3 * (Ga + 2.f * x * Gb + y * Gc);
    gsum += w_l1 / n3 * (float)((d > 0.f) - (d < 0.f));
    gsum += w_l2 * 2.f * d / n3;
    // transposed Sobel: dL/dd(p) = 2/N sum_{u,v} Kx[u][v] gx(p - (u,v)) + Ky[u][v] gy(p - (u,v)), responses outside = 0
    float sob = 0.f;
#pragma unroll
    for (int u = -1; u <= 1; ++u)
#pragma unroll
      for (int w = -1; w <= 1; ++w) {
        const int yy = gy - u, xx = gx - w;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const float kx = (w == 0) ? 0.f : ((w < 0 ? 1.f : -1.f) * (u == 0 ? 2.f : 1.f));
        const float ky = (u == 0) ? 0.f : ((u < 0 ? 1.f : -1.f) * (w == 0 ? 2.f : 1.f));
        const size_t pp = (size_t)yy * W + xx;
        sob += kx * gxy[pp] + ky * gxy[plane + pp];
      }
    gsum += w_sobel * 2.f / n1 * sob;
    if constexpr (MASKED) gsum *= m;   // dx'/dx = m
    grad[ch * plane + p] = gsum;
  }
}

// dst = (src*m + 1) - m (forward) or src*m (backward: the gradient w.r.t. src) over [channels, H, W], one mask value per pixel.
__global__ __launch_bounds__(256) void mask_composite_kernel(int W, int H, int channels, const float* __restrict__ src,
                                                             Mask mk, int backward, float* __restrict__ dst) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const float m = mask_at(mk, y, x);
  const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
  for (int c = 0; c < channels; ++c) dst[c * plane + p] = backward ? src[c * plane + p] * m : composite(src[c * plane + p], m);
}

// ---- geometry loss: the student's depth / alpha maps against the teacher's depth / weight maps ----
// Per pixel: m = up(w), q = up(w * z) with z the teacher's ray distance turned into view-space z at the teacher's cell,
// r_m = A - m, r_d = m*D - A*q; the terms are mean|r_m| and mean|r_d|.  Two launches: the pixel kernel writes both gradient
// maps (their scale is known up front) and one partial sum per workgroup and term; the finalise adds the partials in a fixed
// order.  No atomics: bit-identical from run to run.

struct GeomTeacher { const float* t; Mask w; float tanx, tany; int ray_depth; };

// the premultiplied view-space depth p = w * z of one teacher cell
__device__ __forceinline__ float teacher_p(const GeomTeacher& g, int i, int j) {
  const size_t c = (size_t)i * g.w.w + j;
  float z = g.t[c];
  if (g.ray_depth) {
    const float xl = (2.f * ((float)j + 0.5f) / (float)g.w.w - 1.f) * g.tanx;
    const float yl = (2.f * ((float)i + 0.5f) / (float)g.w.h - 1.f) * g.tany;
    z = z / sqrtf(1.f + xl * xl + yl * yl);
  }
  return g.w.m[c] * z;
}

__device__ __forceinline__ float sign_of(float v) { return (float)((v > 0.f) - (v < 0.f)); }

__global__ __launch_bounds__(256) void geometry_loss_kernel(int W, int H, const float* __restrict__ depth,
                                                            const float* __restrict__ alpha, GeomTeacher g, float s_mask,
                                                            float s_depth, float* __restrict__ grad_depth,
                                                            float* __restrict__ grad_alpha, float* __restrict__ partials) {
  __shared__ float red[4];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  float a_m = 0.f, a_d = 0.f;
  if (x < W && y < H) {
    const MaskAxis ay = mask_axis(y, g.w.fy, g.w.h), ax = mask_axis(x, g.w.fx, g.w.w);
    const float m = mask_value(g.w, ay, ax);
    const float q = mask_blend(teacher_p(g, ay.i0, ax.i0), teacher_p(g, ay.i0, ax.i1), teacher_p(g, ay.i1, ax.i0),
                               teacher_p(g, ay.i1, ax.i1), ay, ax);
    const size_t p = (size_t)y * W + x;
    const float D = depth[p], A = alpha[p];
    const float r_m = A - m, r_d = m * D - A * q;
    const float sm = sign_of(r_m), sd = sign_of(r_d);
    grad_depth[p] = s_depth * sd * m;
    grad_alpha[p] = s_mask * sm - s_depth * sd * q;
    a_m = fabsf(r_m); a_d = fabsf(r_d);
  }
  const float t_m = block_sum(a_m, red), t_d = block_sum(a_d, red);
  if (threadIdx.x == 0) {
    const int wg = blockIdx.y * gridDim.x + blockIdx.x, n_wg = gridDim.x * gridDim.y;
    partials[wg] = t_m; partials[n_wg + wg] = t_d;
  }
}

// one workgroup: lane t adds partials t, t + 256, ... in that order, then the block's fixed tree
__global__ __launch_bounds__(256) void geometry_loss_finalise_kernel(int n_wg, const float* __restrict__ partials, float n_pix,
                                                                     float w_mask, float w_depth, float* __restrict__ terms) {
  __shared__ float red[4];
  float a_m = 0.f, a_d = 0.f;
  for (int i = threadIdx.x; i < n_wg; i += 256) { a_m += partials[i]; a_d += partials[n_wg + i]; }
  const float t_m = block_sum(a_m, red), t_d = block_sum(a_d, red);
  if (threadIdx.x == 0) {
    const float l_m = t_m / n_pix, l_d = t_d / n_pix;
    terms[0] = l_m; terms[1] = l_d; terms[2] = w_mask * l_m + w_depth * l_d;
  }
}

static inline size_t geometry_loss_workgroups(int32_t W, int32_t H) { return (size_t)((W + 63) / 64) * (size_t)((H + 3) / 4); }

// ---- normal-consistency loss: the blended splat normals against the normals of the depth map's surface ----
// Two launches.  Pass 1, per pixel: the surface normal N_s from the central differences dU, dV of the back-projected expected depth
// of the four axis neighbours, e = A - N_r . N_s, dL/dN_r, the direct part of dL/dA, and dL/ddU, dL/ddV into tmp (zeros wherever the
// pixel is not valid); one partial sum of e per workgroup.  Pass 2, per pixel: dL/dP gathered from the four neighbours' dL/ddU, dL/ddV
// (the transposed stencil, so nothing is scattered), chained through P = (x D, y D, D), D = depth / A; its first workgroup adds the
// partials in a fixed order.  No atomics: bit-identical from run to run.

struct NormalCam { int W, H; float tanx, tany, alpha_min; };
struct Vec3 { float x, y, z; };

__device__ __forceinline__ Vec3 cross3(const Vec3 a, const Vec3 b) {
  return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float pixel_x(const NormalCam& c, int x) { return (2.f * ((float)x + 0.5f) / (float)c.W - 1.f) * c.tanx; }
__device__ __forceinline__ float pixel_y(const NormalCam& c, int y) { return (2.f * ((float)y + 0.5f) / (float)c.H - 1.f) * c.tany; }
// the back-projected point of pixel (x, y), whose alpha a is above alpha_min
__device__ __forceinline__ Vec3 pixel_point(const NormalCam& c, const float* __restrict__ depth, int x, int y, float a) {
  const float D = depth[(size_t)y * c.W + x] / a;
  return Vec3{pixel_x(c, x) * D, pixel_y(c, y) * D, D};
}

__global__ __launch_bounds__(256) void normal_loss_pixel_kernel(NormalCam c, const float* __restrict__ normals,
                                                                const float* __restrict__ depth, const float* __restrict__ alpha,
                                                                float inv_n, float* __restrict__ grad_normals,
                                                                float* __restrict__ grad_alpha, float* __restrict__ surface_normals,
                                                                float* __restrict__ guv, float* __restrict__ partials) {
  __shared__ float red[4];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int W = c.W, H = c.H;
  float e = 0.f;
  if (x < W && y < H) {
    const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
    Vec3 ns{0.f, 0.f, 0.f}, gdu{0.f, 0.f, 0.f}, gdv{0.f, 0.f, 0.f};
    bool valid = x > 0 && x < W - 1 && y > 0 && y < H - 1;
    float a = 0.f, al = 0.f, ar = 0.f, au = 0.f, ad = 0.f;
    if (valid) {
      a = alpha[p]; al = alpha[p - 1]; ar = alpha[p + 1]; au = alpha[p - W]; ad = alpha[p + W];
      valid = a > c.alpha_min && al > c.alpha_min && ar > c.alpha_min && au > c.alpha_min && ad > c.alpha_min;
    }
    if (valid) {
      const Vec3 pl = pixel_point(c, depth, x - 1, y, al), pr = pixel_point(c, depth, x + 1, y, ar);
      const Vec3 pu = pixel_point(c, depth, x, y - 1, au), pd = pixel_point(c, depth, x, y + 1, ad);
      const Vec3 dU{pr.x - pl.x, pr.y - pl.y, pr.z - pl.z}, dV{pd.x - pu.x, pd.y - pu.y, pd.z - pu.z};
      const Vec3 cr = cross3(dV, dU);   // faces the camera: (0, 0, -1) on a fronto-parallel plane
      const float len = sqrtf((cr.x * cr.x + cr.y * cr.y) + cr.z * cr.z);
      const Vec3 nr{normals[p], normals[plane + p], normals[2 * plane + p]};
      float dot = 0.f;
      if (len > 0.f) {
        ns = Vec3{cr.x / len, cr.y / len, cr.z / len};
        dot = (nr.x * ns.x + nr.y * ns.y) + nr.z * ns.z;
        // dL/dc through N_s = c / |c|: -(N_r - N_s (N_s . N_r)) / (|c| H W)
        const Vec3 gc{-inv_n * ((nr.x - ns.x * dot) / len), -inv_n * ((nr.y - ns.y * dot) / len),
                      -inv_n * ((nr.z - ns.z * dot) / len)};
        gdv = cross3(dU, gc); gdu = cross3(gc, dV);   // c = dV x dU
      }
      e = a - dot;
    }
    // (0 - ...: a pixel that is not valid gets +0, not -0)
    grad_normals[p] = 0.f - inv_n * ns.x; grad_normals[plane + p] = 0.f - inv_n * ns.y;
    grad_normals[2 * plane + p] = 0.f - inv_n * ns.z;
    grad_alpha[p] = valid ? inv_n : 0.f;
    if (surface_normals) { surface_normals[p] = ns.x; surface_normals[plane + p] = ns.y; surface_normals[2 * plane + p] = ns.z; }
    guv[p] = gdu.x; guv[plane + p] = gdu.y; guv[2 * plane + p] = gdu.z;
    guv[3 * plane + p] = gdv.x; guv[4 * plane + p] = gdv.y; guv[5 * plane + p] = gdv.z;
  }
  const float t = block_sum(e, red);
  if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void normal_loss_gather_kernel(NormalCam c, const float* __restrict__ depth,
                                                                 const float* __restrict__ alpha, const float* __restrict__ guv,
                                                                 const float* __restrict__ partials, int n_wg, float n_pix,
                                                                 float* __restrict__ grad_depth, float* __restrict__ grad_alpha,
                                                                 float* __restrict__ term) {
  __shared__ float red[4];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int W = c.W, H = c.H;
  if (x < W && y < H) {
    const size_t plane = (size_t)H * W, p = (size_t)y * W + x;
    const float a = alpha[p];
    float gd = 0.f;
    if (a > c.alpha_min) {   // (elsewhere no valid pixel has this one as a neighbour: every term below is zero)
      float g[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {   // P(p) is the right point of its left neighbour's dU, the left point of its right one's, ...
        const float* du = guv + k * plane;
        const float* dv = guv + (3 + k) * plane;
        const float l = x > 0 ? du[p - 1] : 0.f, r = x < W - 1 ? du[p + 1] : 0.f;
        const float u = y > 0 ? dv[p - W] : 0.f, d = y < H - 1 ? dv[p + W] : 0.f;
        g[k] = ((l - r) + u) - d;
      }
      const float gD = (pixel_x(c, x) * g[0] + pixel_y(c, y) * g[1]) + g[2];
      gd = gD / a;
      grad_alpha[p] = grad_alpha[p] - gd * (depth[p] / a);
    }
    grad_depth[p] = gd;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {   // lane t adds partials t, t + 256, ... in that order, then the block's fixed tree
    float s = 0.f;
    for (int i = threadIdx.x; i < n_wg; i += 256) s += partials[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) term[0] = t / n_pix;
  }
}

}  // namespace

extern "C" size_t ggd_normal_loss_tmp_bytes(int32_t W, int32_t H) {
  if (W <= 0 || H <= 0) return 0;
  // one partial per workgroup | dL/ddU and dL/ddV, three planes each
  return ggd_align(geometry_loss_workgroups(W, H) * sizeof(float)) + ggd_align((size_t)6 * H * W * sizeof(float));
}

extern "C" int ggd_normal_loss(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* normals, const float* depth,
                               const float* alpha, float tanfovx, float tanfovy, float alpha_min, float* term,
                               float* grad_normals, float* grad_depth, float* grad_alpha, float* surface_normals, void* tmp,
                               size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (W <= 0 || H <= 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_normal_loss: empty image");
  if (!normals || !depth || !alpha || !term || !grad_normals || !grad_depth || !grad_alpha || !tmp)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_normal_loss: NULL pointer");
  if (!(alpha_min >= 0.f)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_normal_loss: alpha_min must not be negative");
  if (tmp_bytes < ggd_normal_loss_tmp_bytes(W, H)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_normal_loss: tmp too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const NormalCam c{W, H, tanfovx, tanfovy, alpha_min};
  const float n_pix = (float)H * (float)W;
  const size_t n_wg = geometry_loss_workgroups(W, H);
  const dim3 grid((W + 63) / 64, (H + 3) / 4);
  float* partials = static_cast<float*>(tmp);
  float* guv = reinterpret_cast<float*>(static_cast<char*>(tmp) + ggd_align(n_wg * sizeof(float)));
  hipLaunchKernelGGL(normal_loss_pixel_kernel, grid, dim3(256), 0, s, c, normals, depth, alpha, 1.f / n_pix, grad_normals,
                     grad_alpha, surface_normals, guv, partials);
  hipLaunchKernelGGL(normal_loss_gather_kernel, grid, dim3(256), 0, s, c, depth, alpha, guv, partials, (int)n_wg, n_pix,
                     grad_depth, grad_alpha, term);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" size_t ggd_geometry_loss_tmp_bytes(int32_t W, int32_t H) {
  if (W <= 0 || H <= 0) return 0;
  return ggd_align(2 * geometry_loss_workgroups(W, H) * sizeof(float));   // one partial per workgroup and term
}

extern "C" int ggd_geometry_loss(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* depth, const float* alpha,
                                 const float* teacher_depth, const float* teacher_weights, int32_t tw, int32_t th,
                                 float tanfovx, float tanfovy, int32_t ray_depth, const float* weights2, float* terms3,
                                 float* grad_depth, float* grad_alpha, void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (W <= 0 || H <= 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_geometry_loss: empty image");
  if (!depth || !alpha || !teacher_depth || !teacher_weights || !weights2 || !terms3 || !grad_depth || !grad_alpha || !tmp)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_geometry_loss: NULL pointer");
  if (tw <= 0 || th <= 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_geometry_loss: empty teacher maps");
  if (H % th != 0 || W % tw != 0)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_geometry_loss: the teacher maps' size must divide the image size");
  if (tmp_bytes < ggd_geometry_loss_tmp_bytes(W, H)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_geometry_loss: tmp too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GeomTeacher g{teacher_depth, Mask{teacher_weights, tw, th, (float)(W / tw), (float)(H / th)}, tanfovx, tanfovy, ray_depth};
  const float n_pix = (float)H * (float)W;
  const dim3 grid((W + 63) / 64, (H + 3) / 4);
  float* partials = static_cast<float*>(tmp);
  hipLaunchKernelGGL(geometry_loss_kernel, grid, dim3(256), 0, s, W, H, depth, alpha, g, weights2[0] / n_pix,
                     weights2[1] / n_pix, grad_depth, grad_alpha, partials);
  hipLaunchKernelGGL(geometry_loss_finalise_kernel, dim3(1), dim3(256), 0, s, (int)geometry_loss_workgroups(W, H), partials,
                     n_pix, weights2[0], weights2[1], terms3);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" size_t ggd_image_loss_tmp_bytes(int32_t W, int32_t H) {
  if (W <= 0 || H <= 0) return 0;
  return ggd_align(64) + ggd_align((size_t)11 * H * W * sizeof(float));   // sums | 9 abc maps + 2 Sobel maps
}

// Shared body of ggd_image_loss (mask == nullptr) and ggd_image_loss_masked.
static int image_loss_launch(ggd_ctx* ctx, const char* who, void* stream, int32_t W, int32_t H, const float* image,
                             const float* target, const float* mask, int32_t mask_w, int32_t mask_h, bool masked,
                             const float* weights4, float* terms5, float* grad_image, void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  const std::string name(who);
  if (W <= 0 || H <= 0) return ggd_fail(ctx, GGD_E_INVALID, name + ": empty image");
  if (!image || !target || !weights4 || !terms5 || !grad_image || !tmp || (masked && !mask))
    return ggd_fail(ctx, GGD_E_INVALID, name + ": NULL pointer");
  Mask mk{nullptr, 0, 0, 1.f, 1.f};
  if (masked) {
    if (mask_w <= 0 || mask_h <= 0) return ggd_fail(ctx, GGD_E_INVALID, name + ": empty mask");
    if (H % mask_h != 0 || W % mask_w != 0)
      return ggd_fail(ctx, GGD_E_INVALID, name + ": the mask size must divide the image size");
    mk = Mask{mask, mask_w, mask_h, (float)(W / mask_w), (float)(H / mask_h)};
  }
  if (tmp_bytes < ggd_image_loss_tmp_bytes(W, H)) return ggd_fail(ctx, GGD_E_INVALID, name + ": tmp too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Win win;
  {  // loss_utils.py:23-25: exp(-(x - 5)^2 / (2 sigma^2)) as float32, normalised by its float32 sum
    float g[11], sum = 0.f;
    for (int i = 0; i < 11; ++i) { g[i] = (float)std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    for (int i = 0; i < 11; ++i) win.g[i] = g[i] / sum;
  }
  float* sums = static_cast<float*>(tmp);
  float* abc = reinterpret_cast<float*>(static_cast<char*>(tmp) + ggd_align(64));
  float* gxy = abc + (size_t)9 * H * W;
  GGD_HIP(hipMemsetAsync(sums, 0, 64, s));
  const dim3 tiles((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, 3);
  ggd_dispatch<2>(masked, [&](auto mf) {
    constexpr bool M = decltype(mf)::value != 0;
    hipLaunchKernelGGL(ssim_stats_kernel<M>, tiles, dim3(256), 0, s, W, H, win, image, target, abc, sums, mk);
    hipLaunchKernelGGL(sobel_kernel<M>, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, s, W, H, image, target, gxy, sums, mk);
    hipLaunchKernelGGL(grad_kernel<M>, tiles, dim3(256), 0, s, W, H, win, image, target, abc, gxy, sums, weights4[0],
                       weights4[1], weights4[2], weights4[3], grad_image, terms5, mk);
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_image_loss(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* image,
                              const float* target, const float* weights4, float* terms5, float* grad_image,
                              void* tmp, size_t tmp_bytes) {
  return image_loss_launch(ctx, "ggd_image_loss", stream, W, H, image, target, nullptr, 0, 0, false, weights4, terms5,
                           grad_image, tmp, tmp_bytes);
}

extern "C" int ggd_image_loss_masked(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, const float* image,
                                     const float* target, const float* mask, int32_t mask_w, int32_t mask_h,
                                     const float* weights4, float* terms5, float* grad_image, void* tmp,
                                     size_t tmp_bytes) {
  return image_loss_launch(ctx, "ggd_image_loss_masked", stream, W, H, image, target, mask, mask_w, mask_h, true,
                           weights4, terms5, grad_image, tmp, tmp_bytes);
}

extern "C" int ggd_mask_composite(ggd_ctx* ctx, void* stream, int32_t W, int32_t H, int32_t channels, const float* src,
                                  const float* mask, int32_t mask_w, int32_t mask_h, int32_t backward, float* dst) {
  if (!ctx) return GGD_E_INVALID;
  if (W <= 0 || H <= 0 || channels <= 0 || mask_w <= 0 || mask_h <= 0)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_mask_composite: empty image or mask");
  if (!src || !mask || !dst) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mask_composite: NULL pointer");
  if (H % mask_h != 0 || W % mask_w != 0)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_mask_composite: the mask size must divide the image size");
  const Mask mk{mask, mask_w, mask_h, (float)(W / mask_w), (float)(H / mask_h)};
  hipLaunchKernelGGL(mask_composite_kernel, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0,
                     static_cast<hipStream_t>(stream), W, H, channels, src, mk, backward, dst);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
