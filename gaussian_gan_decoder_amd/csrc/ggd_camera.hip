// ggd_camera.hip -- the camera's gradients (ggd_backward_camera): dL/dviewmatrix, dL/dprojmatrix, dL/dcampos.
//
// One more launch pair behind the per-Gaussian backward, on the same accumulator records (which by then hold the colour, depth /
// alpha, feature and distortion terms together).  Per visible Gaussian, with p = (p0, p1, p2, 1) and the quantities of
// preprocess_backward_body under their names there (the shared pieces are in ggd_math.h), flat entry m[4c + r] = row r, column c:
//   view, through t = V p        dV[4c + r]  += dt_r p_c,  r = 0..2   (dt before its multiplication by V^T; the accumulator's depth
//                                                                      slot joins dt_z in the AUX instances)
//   view, through W in T = J W   dV[4c + 0]  += J00 dT[0][c];  dV[4c + 1] += J11 dT[1][c];  dV[4c + 2] += J02 dT[0][c] + J12 dT[1][c]
//   projection                   dPV[4c + r] += dh_r p_c,  dh = (m_w g0, m_w g1, -, -(mul1 g0 + mul2 g1))
//   camera centre                dcampos     -= the SH view-direction term of dL/dmean (zero at degree 0 and with colors_precomp)
// The bottom row of V and row 2 of PV are read by no kernel: their gradients are exactly 0.  It is the derivative of the surrogate
// the means' gradient is the derivative of (1/(det^2 + 1e-7), the half dB slot, clamped x, y independent of z).
//
// 27 sums over P, reduced in a fixed order without float atomics: the DPP scan of the wave (ggd_lanes.h), the workgroup's four
// waves through LDS in wave order, one partial row per workgroup in the context's workspace; camera_finish_kernel then sums each
// column -- lane l takes rows l, l + 256, ... in index order, the 256 lanes are joined by the same scan and wave order -- and writes
// all 35 values.  Given the same accumulator records the result is bit-identical from run to run.
#include "ggd_lanes.h"
#include "ggd_math.h"

namespace {
using namespace ggdm;

constexpr int CAM_SUMS = 27;   // 0..11 view (3 c + r, r = 0..2) | 12..23 projection (3 c + j, rows 0, 1, 3) | 24..26 camera centre
constexpr int CAM_WG = 256;

// the sum of v over the workgroup's 256 lanes, valid in thread 0 (wave sums in s_w[4], added in wave order)
__device__ __forceinline__ float workgroup_sum(float v, float* s_w) {
  v = wave_sum_lane63(v);
  if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

template <bool AA = false, bool AUX = false>
__global__ __launch_bounds__(CAM_WG) void camera_partial_kernel(
    int P, int M, int deg, int W, int H, float tanfovx, float tanfovy, float mod, int raw,
    const float* __restrict__ opacities_raw, const float* __restrict__ view, const float* __restrict__ proj,
    const float* __restrict__ campos_p, const float* __restrict__ means3D, const float* __restrict__ shs,
    const float* __restrict__ colors_precomp, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ cov3D_precomp, const int32_t* __restrict__ radii, const uint8_t* __restrict__ clamped,
    const float* __restrict__ grad_acc, float* __restrict__ partial /*[CAM_SUMS][gridDim.x]*/) {
  __shared__ float s_w[CAM_SUMS][4];
  const int i = blockIdx.x * CAM_WG + threadIdx.x;
  float sum[CAM_SUMS];
#pragma unroll
  for (int k = 0; k < CAM_SUMS; ++k) sum[k] = 0.0f;
  // (no early return: every lane takes part in the wave sums below; a culled Gaussian and a lane past P add zeros)
  if (i < P && radii[i] > 0) {
    const size_t ii = (size_t)i;
    const float4 acc0 = reinterpret_cast<const float4*>(grad_acc)[3 * ii];      // conic A, B, C | opacity
    const float4 acc1 = reinterpret_cast<const float4*>(grad_acc)[3 * ii + 1];  // mean2D x, y | colour r, g
    const float4 acc2 = reinterpret_cast<const float4*>(grad_acc)[3 * ii + 2];  // colour b | depth | abs mean2D x, y
    const Mat16 V = load_mat(view);
    const Mat16 PV = load_mat(proj);
    const float p[4] = {means3D[3 * ii], means3D[3 * ii + 1], means3D[3 * ii + 2], 1.0f};
    float c6[6];
    if (cov3D_precomp) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * ii + k];
    } else {
      float s3[3] = {scales[3 * ii], scales[3 * ii + 1], scales[3 * ii + 2]};
      float4 q = reinterpret_cast<const float4*>(rotations)[i];
      if (raw) {
        float q_norm;
        s3[0] = expf(s3[0]); s3[1] = expf(s3[1]); s3[2] = expf(s3[2]);
        q = act_normalize(q, q_norm);
      }
      cov3d_from_scale_rot(s3, mod, q, c6);
    }
    // view: the point t = V p, and W in T = J W
    {
      float t[3];
      t[0] = V.m[0] * p[0] + V.m[4] * p[1] + V.m[8] * p[2] + V.m[12];
      t[1] = V.m[1] * p[0] + V.m[5] * p[1] + V.m[9] * p[2] + V.m[13];
      t[2] = V.m[2] * p[0] + V.m[6] * p[1] + V.m[10] * p[2] + V.m[14];
      const float fx = (float)W / (2.0f * tanfovx), fy = (float)H / (2.0f * tanfovy);
      float abc[3], T[2][3], tc[3];
      bool clx, cly;
      ewa_cov2d(t, fx, fy, tanfovx, tanfovy, c6, V, abc, T, tc, clx, cly);
      float aa_o = 0.0f, aa_h = 1.0f;
      if constexpr (AA) aa_o = raw ? act_sigmoid(opacities_raw[i]) : opacities_raw[i];
      float dL_da, dL_db, dL_dc;
      cov2d_backward<AA>(abc, acc0.x, acc0.y, acc0.z, acc0.w, aa_o, aa_h, dL_da, dL_db, dL_dc);
      float dT[2][3], dt[3];
      ewa_dT(T, c6, dL_da, dL_db, dL_dc, dT);
      ewa_dt(V, dT, fx, fy, tc, clx, cly, dt);
      if constexpr (AUX) {
        static_assert(GGD_ACC_DEPTH == 9, "depth gradient is read from acc2.y");
        dt[2] += acc2.y;
      }
      float J00, J02, J11, J12;
      ewa_jacobian(tc, fx, fy, J00, J02, J11, J12);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;
        if (c < 3) { w0 = J00 * dT[0][c]; w1 = J11 * dT[1][c]; w2 = J02 * dT[0][c] + J12 * dT[1][c]; }
        sum[3 * c + 0] = dt[0] * p[c] + w0;
        sum[3 * c + 1] = dt[1] * p[c] + w1;
        sum[3 * c + 2] = dt[2] * p[c] + w2;
      }
    }
    // projection: the screen position through the perspective divide
    {
      float m_w, mul1, mul2;
      divide_terms(PV, p, m_w, mul1, mul2);
      const float g0 = acc1.x, g1 = acc1.y;
      const float dh0 = m_w * g0, dh1 = m_w * g1, dh3 = -(mul1 * g0 + mul2 * g1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        sum[12 + 3 * c + 0] = dh0 * p[c];
        sum[12 + 3 * c + 1] = dh1 * p[c];
        sum[12 + 3 * c + 2] = dh3 * p[c];
      }
    }
    // camera centre: the colour through the SH view direction
    if (!colors_precomp && deg > 0) {
      const float gcol3[3] = {acc1.z, acc1.w, acc2.x};
      const float* sh = shs + ii * M * 3;
      const uint32_t cl = clamped[i];
      const float v[3] = {p[0] - campos_p[0], p[1] - campos_p[1], p[2] - campos_p[2]};
      const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      const float x = v[0] / len, y = v[1] / len, z = v[2] / len;
      float ddir[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float gcol = ((cl >> c) & 1u) ? 0.0f : gcol3[c];
        float dx, dy, dz;
        sh_dir_grad(deg, sh, c, x, y, z, dx, dy, dz);
        ddir[0] += dx * gcol; ddir[1] += dy * gcol; ddir[2] += dz * gcol;
      }
      float dv[3];
      dir_to_point(v, ddir, dv);
      sum[24] = -dv[0]; sum[25] = -dv[1]; sum[26] = -dv[2];
    }
  }
#pragma unroll
  for (int k = 0; k < CAM_SUMS; ++k) {
    const float v = wave_sum_lane63(sum[k]);
    if ((threadIdx.x & 63) == 63) s_w[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < CAM_SUMS) {
    const float* w = s_w[threadIdx.x];
    partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
  }
}

// One workgroup per output value: 0..15 dL_dviewmatrix, 16..31 dL_dprojmatrix, 32..34 dL_dcampos.  Every value is written, the
// entries no kernel reads as zeros.
__global__ __launch_bounds__(CAM_WG) void camera_finish_kernel(const float* __restrict__ partial, int rows,
                                                               float* __restrict__ dL_dview, float* __restrict__ dL_dproj,
                                                               float* __restrict__ dL_dcampos) {
  __shared__ float s_w[4];
  const int o = blockIdx.x;
  int k;        // the column of `partial`, -1: none
  float* dst;
  if (o < 16) { const int r = o & 3, c = o >> 2; k = r < 3 ? 3 * c + r : -1; dst = dL_dview + o; }
  else if (o < 32) { const int r = o & 3, c = (o - 16) >> 2; k = r == 2 ? -1 : 12 + 3 * c + (r == 3 ? 2 : r); dst = dL_dproj + (o - 16); }
  else { k = 24 + (o - 32); dst = dL_dcampos + (o - 32); }
  float acc = 0.0f;
  if (k >= 0)
    for (int j = threadIdx.x; j < rows; j += CAM_WG) acc += partial[(size_t)k * rows + j];
  const float total = workgroup_sum(acc, s_w);
  if (threadIdx.x == 0) *dst = k >= 0 ? total : 0.0f;
}

int ggd_camera_partial_rows(int P) { return (P + CAM_WG - 1) / CAM_WG; }   // workgroups of the partial kernel = rows of `partial`

}  // namespace

size_t ggd_camera_tmp_bytes(int P) { return (size_t)ggd_camera_partial_rows(P) * CAM_SUMS * sizeof(float); }

int ggd_launch_camera_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_inputs& in, const int32_t* radii,
                               const uint8_t* clamped, const float* grad_acc, bool aux, float* partial,
                               const ggd_camera_grads& out) {
  const int rows = ggd_camera_partial_rows(prm.P);
  ggd_dispatch<2>(prm.antialiasing != 0, [&](auto aa) {
    ggd_dispatch<2>(aux, [&](auto ax) {
      constexpr bool AA = decltype(aa)::value != 0, AUX = decltype(ax)::value != 0;
      hipLaunchKernelGGL((camera_partial_kernel<AA, AUX>), dim3(rows), dim3(CAM_WG), 0, s, prm.P, prm.M, prm.sh_degree, prm.width,
                         prm.height, prm.tanfovx, prm.tanfovy, prm.scale_modifier, prm.raw_attributes, in.opacities,
                         prm.viewmatrix, prm.projmatrix, prm.campos, in.means3D, in.shs, in.colors_precomp, in.scales,
                         in.rotations, in.cov3D_precomp, radii, clamped, grad_acc, partial);
    });
  });
  GGD_HIP(hipGetLastError());
  hipLaunchKernelGGL(camera_finish_kernel, dim3(35), dim3(CAM_WG), 0, s, partial, rows, out.dL_dviewmatrix, out.dL_dprojmatrix,
                     out.dL_dcampos);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
