// ggd_density.hip -- the teacher's density (and colour) field sampled on the device: feature planes -> sigma [, rgb] per point,
// one launch, nothing but the results written to memory.
//
// What the reference does every iteration with G.sample_mixed (main/decoder_utils/target_dataloader.py:134-169) in 1 M-point
// chunks: sample_from_planes (eg3d / PanoHead training/volumetric_rendering/renderer.py) -> OSGDecoder (training/triplane.py:
// mean over the three planes, FullyConnectedLayer 32 -> 64, softplus, FullyConnectedLayer 64 -> 1 + 32, the rgb activation),
// on the lattice of main/marching_cube/sample.py:5-26 (create_samples).
//
// Per point:   f = mean over the planes of the bilinear / trilinear sample   (the expressions of gather4_kernel, ggd_triplane.hip)
//              h = softplus(W1 f + b1)                                       (64 wide)
//              sigma = W2[0] . h + b2[0];   rgb = act(W2[1:33] h + b2[1:33]) (rgb only in the RGB instances)
// All fp32: the sigma is thresholded at 10 downstream.
//
// Layout.  A workgroup of 4 waves takes DN_POINTS = 128 points, a wave 32 of them -- the 32 columns of the f32-input MFMA
// (v_mfma_f32_32x32x2_f32: an exact k-ordered fp32 FMA chain at the VALU's peak rate, which leaves the VALU to the softplus):
//   gather    8 lanes per point, 16 bytes of a texel line each (as gather4_kernel), 4 passes of 8 points; the features go to
//             an LDS tile [point][channel] of the wave (the gather has the point on lane / 8, the MFMA wants it on lane % 32);
//   layer 1   H^T [64 x 32 points] = W1 [64 x 32] . F^T: two 32-row tiles, 16 k-steps each, the accumulators start at b1.
//             Lane (j = lane % 32, half = lane / 32) reads float4s at channel 8 m + 4 half of its W1 row and of its point's
//             features, so k-step 4 m + e pairs channel 8 m + e (half 0) with channel 8 m + 4 + e (half 1);
//   softplus  on the 32 accumulator registers of the lane (hidden units 32 t + 8 g + 4 half + e, register 4 g + e of tile t);
//   sigma     ONE row next to 32-row tiles: not worth an MFMA tile with 31 idle rows (it would double layer 2).  Each lane
//             takes the dot product over its own 32 hidden units with v_fma_f32, the two halves of a point are added across
//             lanes, then b2[0]: 32 VALU FMAs per lane.  The sigma-only instances stop here and never read W2[1:33];
//   rgb       O [32 x 32 points] = W2[1:33] . H: the accumulator registers of layer 1 ARE the B operand (column on the lane,
//             rows in the registers): k-step 16 t + 4 g + e takes register 4 g + e of tile t, and the A operand the matching
//             column 32 t + 8 g + 4 half + e of W2 -- again one float4 per (t, g).  No transpose, no LDS trip for H.
// Weights and biases are staged in LDS once per workgroup (17 KB, L2 hits) and read as operands from there: the kernel
// keeps ~100 VGPRs and 4 workgroups per CU for the gather's latency.  No atomics; every sum has one fixed order, so results
// are bit-identical from run to run, and the sigma of a sigma-only call is the sigma of a sigma + rgb call.
//
// Coordinates come from pos[N][3] or are generated in registers (DnSrc): the reference's lattice, op for op in fp32, or the
// regular one.
#include "ggd_common.h"
#include "ggd_density_launch.h"
#include "ggd_planes.h"

namespace {

constexpr int DN_C = 32;        // plane channels
constexpr int DN_HID = 64;      // hidden units
constexpr int DN_RGB = 32;      // rgb channels
constexpr int DN_POINTS = 128;  // points per workgroup: 4 waves x the 32 columns of an MFMA tile
constexpr int DN_ROW = DN_C + 4;     // floats per LDS row of 32 (W1 rows, feature rows): float4-aligned, rows on different banks
constexpr int DN_ROW2 = DN_HID + 4;  // floats per LDS row of W2
constexpr int DN_MAX_N = 1024;  // lattice samples per axis (n^3 <= 2^30 fits the int32 sample index)

using f32x16 = __attribute__((ext_vector_type(16))) float;

// Where the coordinates come from.  mode 0: pos[N][3];  1: the reference's lattice (create_samples: un-floored float
// division, so the y and x indices carry fractional parts);  2: the regular lattice (floored indices).
struct DnSrc { const float* pos; int mode; int n; float voxel, origin; };

// Sample i of the n^3 lattice.  mode 1 repeats main/marching_cube/sample.py:15-23 in fp32, op for op:
//   t_z = i mod n,  t_y = fmod(float(i) / n, n),  t_x = fmod((float(i) / n) / n, n),  coordinate = fl(fl(t * voxel) + origin)
// (IEEE division; the multiply and the add are the rounding intrinsics, which no contraction can fuse).
__device__ __forceinline__ void lattice_xyz(int mode, int n, float voxel, float origin, int i, float& x, float& y, float& z) {
  const float fn = (float)n;
  float tx, ty;
  const float tz = (float)(i % n);
  if (mode == 1) {
    const float q = (float)i / fn;
    ty = fmodf(q, fn);
    tx = fmodf(q / fn, fn);
  } else {
    ty = (float)((i / n) % n);
    tx = (float)(i / (n * n));
  }
  x = __fadd_rn(__fmul_rn(tx, voxel), origin);
  y = __fadd_rn(__fmul_rn(ty, voxel), origin);
  z = __fadd_rn(__fmul_rn(tz, voxel), origin);
}

__device__ __forceinline__ void source_xyz(const DnSrc& src, int64_t i, float& x, float& y, float& z) {
  if (src.mode == 0) { x = src.pos[3 * i]; y = src.pos[3 * i + 1]; z = src.pos[3 * i + 2]; }
  else lattice_xyz(src.mode, src.n, src.voxel, src.origin, (int)i, x, y, z);
}

// torch's softplus (beta 1, threshold 20).  log1pf(expf(z)) keeps the relative accuracy of e^z for very negative z, which
// log(1 + exp) on the fast intrinsics would round to 0.
__device__ __forceinline__ float dn_softplus(float z) { return z > 20.0f ? z : log1pf(expf(z)); }

// rgb activations of OSGDecoder.  0: sigmoid * 1.002 - 0.001 (EG3D; PanoHead "sigmoid"), 1: leaky_relu(0.2) * sqrt(2), 2: none
__device__ __forceinline__ float dn_act(int act, float v) {
  if (act == 0) return (1.0f / (1.0f + expf(-v))) * 1.002f - 0.001f;
  if (act == 1) return (v > 0.0f ? v : v * 0.2f) * 1.41421356237309515f;
  return v;
}

// The mean over the three planes of the point's sample, channels 4 q .. 4 q + 3: gather4_kernel (ggd_triplane.hip) without the
// modulation.  Shared with it, through ggd_planes.h: the cell, and the coordinates, inside test, weight and texel of each tap.
// NOT shared: the loop around them (request every tap, then sum the inside ones) -- one per-point function called by both
// kernels compiled to other instruction streams in both (density_kernel<true, *>: 156 -> 160 VGPRs), and so did taking the
// tap's coordinates after the inside test instead of before it.  To re-check after a change here or in
// ggd_planes.h: python scripts/kernel_diff.py OLD NEW over two builds; gather4_kernel and density_kernel must report `same`.
template <bool G3>
__device__ __forceinline__ float4 dn_gather(const float* __restrict__ grids_cl, int D, int H, int W, int axes, float x, float y,
                                            float z, int q) {
  constexpr int C = DN_C;
  const int Dd = G3 ? D : 1;
  const size_t grid_stride = (size_t)Dd * H * W * C;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const PlaneCell cell = plane_cell<G3>(axes, p, x, y, z, D, H, W);
    const PlaneTap corner = cell_corner<G3>(cell);
    float4 t[G3 ? 8 : 4];   // all taps of the plane are requested before the first is used
    float wg[G3 ? 8 : 4];
    bool ins[G3 ? 8 : 4];
#pragma unroll
    for (int k = 0; k < (G3 ? 8 : 4); ++k) {
      const PlaneTap tap = tap_at<G3>(corner, k);
      const bool in = tap_in<G3>(cell, k, Dd, H, W);
      wg[k] = tap_weight<G3>(cell, k);
      ins[k] = in;
      t[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (in) t[k] = *reinterpret_cast<const float4*>(grids_cl + p * grid_stride + tap_texel(tap, H, W) * C + 4 * q);
    }
#pragma unroll
    for (int k = 0; k < (G3 ? 8 : 4); ++k) {
      if (ins[k]) {   // an outside tap adds nothing: skipped, as the gather skips it (a NaN weight cannot reach the sum)
        acc.x += wg[k] * t[k].x; acc.y += wg[k] * t[k].y; acc.z += wg[k] * t[k].z; acc.w += wg[k] * t[k].w;
      }
    }
  }
  const float third = 1.0f / 3.0f;
  return make_float4(acc.x * third, acc.y * third, acc.z * third, acc.w * third);
}

template <bool G3, bool RGB>
__global__ __launch_bounds__(256, 3) void density_kernel(const float* __restrict__ grids_cl, int D, int H, int W, int axes,
                                                      float scale, const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, int act,
                                                      DnSrc src, int64_t N, float* __restrict__ sigma, float* __restrict__ rgb) {
  constexpr int ROWS2 = RGB ? 1 + DN_RGB : 1;   // rows of W2 / b2 this instance reads
  __shared__ __align__(16) float s_w1[DN_HID * DN_ROW];
  __shared__ __align__(16) float s_w2[ROWS2 * DN_ROW2];
  __shared__ __align__(16) float s_f[4][32 * DN_ROW];
  __shared__ float s_b1[DN_HID];
  __shared__ float s_b2[ROWS2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < DN_HID * DN_C; i += 256) s_w1[(i / DN_C) * DN_ROW + (i % DN_C)] = w1[i];
  for (int i = tid; i < ROWS2 * DN_HID; i += 256) s_w2[(i / DN_HID) * DN_ROW2 + (i % DN_HID)] = w2[i];
  if (tid < DN_HID) s_b1[tid] = b1[tid];
  if (tid < ROWS2) s_b2[tid] = b2[tid];

  // ---- gather: 8 lanes per point, 4 passes of 8 points -> the wave's feature tile [32 points][32 channels] ----------------
  const int64_t wbase = (int64_t)blockIdx.x * DN_POINTS + wv * 32;
  {
    const int q = lane & 7;
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
      const int jl = 8 * r + (lane >> 3);
      const int64_t n = wbase + jl;
      float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (n < N) {
        float px, py, pz;
        source_xyz(src, n, px, py, pz);
        f = dn_gather<G3>(grids_cl, D, H, W, axes, scale * px, scale * py, scale * pz, q);
      }
      *reinterpret_cast<float4*>(&s_f[wv][jl * DN_ROW + 4 * q]) = f;
    }
  }
  __syncthreads();
  if (wbase >= N) return;

  // ---- layer 1 on the MFMA: accumulator register v of tile t = hidden unit 32 t + 8 (v / 4) + 4 half + v % 4 of point j ----
  const int j = lane & 31, half = lane >> 5;
  f32x16 h[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) h[t][v] = s_b1[32 * t + 8 * (v >> 2) + 4 * half + (v & 3)];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const float4 bf = *reinterpret_cast<const float4*>(&s_f[wv][j * DN_ROW + 8 * m + 4 * half]);
    const float bfe[4] = {bf.x, bf.y, bf.z, bf.w};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 a = *reinterpret_cast<const float4*>(&s_w1[(32 * t + j) * DN_ROW + 8 * m + 4 * half]);
      const float ae[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) h[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], bfe[e], h[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) h[t][v] = dn_softplus(h[t][v]);

  const int64_t n = wbase + j;
  // ---- sigma: the lane's 32 hidden units on the VALU, the two halves of the point added across lanes ------------------------
  {
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 w = *reinterpret_cast<const float4*>(&s_w2[32 * t + 8 * g + 4 * half]);
        s = __builtin_fmaf(w.x, h[t][4 * g], s); s = __builtin_fmaf(w.y, h[t][4 * g + 1], s);
        s = __builtin_fmaf(w.z, h[t][4 * g + 2], s); s = __builtin_fmaf(w.w, h[t][4 * g + 3], s);
      }
    const float other = __shfl_xor(s, 32);
    const float lo = half ? other : s, hi = half ? s : other;   // the same sum in both lanes of the point
    if (half == 0 && n < N) sigma[n] = (lo + hi) + s_b2[0];
  }

  // ---- rgb on the MFMA: layer 1's accumulator registers are the B operand ---------------------------------------------------
  if constexpr (RGB) {
    f32x16 o;
#pragma unroll
    for (int v = 0; v < 16; ++v) o[v] = s_b2[1 + 8 * (v >> 2) + 4 * half + (v & 3)];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(&s_w2[(1 + j) * DN_ROW2 + 32 * t + 8 * g + 4 * half]);
        const float ae[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], h[t][4 * g + e], o, 0, 0, 0);
      }
    if (n < N) {
#pragma unroll
      for (int g = 0; g < 4; ++g)   // register 4 g + e = channel 8 g + 4 half + e
        *reinterpret_cast<float4*>(rgb + n * DN_RGB + 8 * g + 4 * half) =
            make_float4(dn_act(act, o[4 * g]), dn_act(act, o[4 * g + 1]), dn_act(act, o[4 * g + 2]), dn_act(act, o[4 * g + 3]));
    }
  }
}

__global__ __launch_bounds__(256) void lattice_kernel(int mode, int n, float voxel, float origin, int total,
                                                      float* __restrict__ pos) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float x, y, z;
  lattice_xyz(mode, n, voxel, origin, i, x, y, z);
  pos[3 * (size_t)i] = x; pos[3 * (size_t)i + 1] = y; pos[3 * (size_t)i + 2] = z;
}

// voxel and origin as the reference forms them: in double, then rounded to fp32 by the tensor arithmetic that uses them
bool lattice_source(int n, double cube_length, int lattice, DnSrc& src) {
  if (n < 2 || n > DN_MAX_N || lattice < 0 || lattice > 1 || !(cube_length > 0.0)) return false;
  src.pos = nullptr;
  src.mode = lattice == 0 ? 1 : 2;
  src.n = n;
  src.voxel = (float)(cube_length / (double)(n - 1));
  src.origin = (float)(-cube_length / 2.0);
  return true;
}

int launch_density(ggd_ctx* ctx, hipStream_t s, const char* who, const ggd_plane_set& ps, const ggd_field_weights& fw,
                   const DnSrc& src, int64_t N, float* sigma, float* rgb) {
  const int rc = ggd_check_field(ctx, who, ps, fw);
  if (rc != GGD_OK) return rc;
  if (N <= 0) return GGD_OK;
  if (!ps.grids_cl || !fw.w1 || !fw.b1 || !fw.w2 || !fw.b2 || !sigma || ps.H <= 0 || ps.W <= 0 || ps.box_warp == 0.0f)
    return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": bad argument");
  const float scale = 2.0f / ps.box_warp;
  const dim3 grid((unsigned)((N + DN_POINTS - 1) / DN_POINTS));
  ggd_dispatch<2>(ps.D > 0, [&](auto g3) {
    ggd_dispatch<2>(rgb != nullptr, [&](auto want_rgb) {
      hipLaunchKernelGGL((density_kernel<decltype(g3)::value != 0, decltype(want_rgb)::value != 0>), grid, dim3(256), 0, s,
                         ps.grids_cl, ps.D, ps.H, ps.W, ps.axes, scale, fw.w1, fw.b1, fw.w2, fw.b2, fw.act, src, N, sigma, rgb);
    });
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

}  // namespace

int ggd_check_field(ggd_ctx* ctx, const char* who, const ggd_plane_set& ps, const ggd_field_weights& fw) {
  if (ps.C != DN_C) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": 32 plane channels, 64 hidden units and 32 rgb channels only");
  const int rc = ggd_check_plane_set(ctx, who, ps);
  if (rc != GGD_OK) return rc;
  if (fw.act < 0 || fw.act > 2) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": rgb_act is 0 (sigmoid), 1 (lrelu) or 2 (none)");
  return GGD_OK;
}

int ggd_launch_density_points(ggd_ctx* ctx, hipStream_t s, const char* who, const ggd_plane_set& ps, const ggd_field_weights& fw,
                              const float* pos, int64_t N, float* sigma, float* rgb) {
  return launch_density(ctx, s, who, ps, fw, DnSrc{pos, 0, 0, 0.0f, 0.0f}, N, sigma, rgb);
}

extern "C" int ggd_density_points(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                                  int32_t axes, float box_warp, const float* w1, const float* b1, const float* w2,
                                  const float* b2, int32_t rgb_act, const float* pos, int32_t N, float* sigma, float* rgb) {
  if (!ctx) return GGD_E_INVALID;
  if (N > 0 && !pos) return ggd_fail(ctx, GGD_E_INVALID, "ggd_density_points: bad argument");
  const ggd_plane_set ps = {.grids_cl = grids_cl, .C = C, .D = D, .H = H, .W = W, .axes = axes, .box_warp = box_warp};
  const ggd_field_weights fw = {.w1 = w1, .b1 = b1, .w2 = w2, .b2 = b2, .act = rgb_act};
  return ggd_launch_density_points(ctx, static_cast<hipStream_t>(stream), "ggd_density_points", ps, fw, pos, N, sigma, rgb);
}

extern "C" int ggd_density_grid(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H, int32_t W,
                                int32_t axes, float box_warp, const float* w1, const float* b1, const float* w2,
                                const float* b2, int32_t rgb_act, int32_t n, double cube_length, int32_t lattice, float* sigma,
                                float* rgb) {
  if (!ctx) return GGD_E_INVALID;
  DnSrc src;
  if (!lattice_source(n, cube_length, lattice, src))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_density_grid: 2 <= n <= 1024, cube_length > 0, lattice 0 (reference) or 1 (regular)");
  const ggd_plane_set ps = {.grids_cl = grids_cl, .C = C, .D = D, .H = H, .W = W, .axes = axes, .box_warp = box_warp};
  const ggd_field_weights fw = {.w1 = w1, .b1 = b1, .w2 = w2, .b2 = b2, .act = rgb_act};
  return launch_density(ctx, static_cast<hipStream_t>(stream), "ggd_density_grid", ps, fw, src, (int64_t)n * n * n, sigma, rgb);
}

extern "C" int ggd_density_lattice(ggd_ctx* ctx, void* stream, int32_t n, double cube_length, int32_t lattice, float* pos) {
  if (!ctx) return GGD_E_INVALID;
  DnSrc src;
  if (!lattice_source(n, cube_length, lattice, src) || !pos)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_density_lattice: 2 <= n <= 1024, cube_length > 0, lattice 0 (reference) or 1 (regular)");
  const int total = n * n * n;
  hipLaunchKernelGGL(lattice_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src.mode,
                     n, src.voxel, src.origin, total, pos);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
