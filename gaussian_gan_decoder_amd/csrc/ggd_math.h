// ggd_math.h -- per-Gaussian device math shared by the forward and backward preprocess kernels.
// fp32, evaluated exactly as written (-ffp-contract=off); the operation order is part of the parity contract
// (radii / tiles_touched / depth bits are bit-exact anchors), see SURVEY.md section 9.2.
#pragma once
#include "ggd_common.h"

namespace ggdm {

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
__device__ constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                       -1.0925484305920792f, 0.5462742152960396f};
__device__ constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                       0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                                       -0.5900435899266435f};

struct Mat16 { float m[16]; };

// Camera matrices / bg / campos are small read-only device arrays written before the launch: read them through
// the constant address space so the wave-uniform loads become s_load (SGPRs, scalar cache) instead of 16 VMEM
// loads per lane.
typedef const __attribute__((address_space(4))) float* ggd_cptr;
__device__ __forceinline__ ggd_cptr as_const(const float* p) { return (ggd_cptr)(unsigned long long)p; }

__device__ __forceinline__ Mat16 load_mat(const float* __restrict__ p) {
  Mat16 r;
  ggd_cptr c = as_const(p);
#pragma unroll
  for (int i = 0; i < 16; ++i) r.m[i] = c[i];
  return r;
}

// Activation prologue of the reference's GaussianModel getters (gaussian_model.py:100-121), fused on request.
__device__ __forceinline__ float act_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float4 act_normalize(float4 q, float& norm) {
  norm = sqrtf((q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w));
  const float d = fmaxf(norm, 1e-12f);  // torch.nn.functional.normalize: v / max(||v||, eps)
  return make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}
// Its Jacobian, transposed: dq = dL/dq_hat -> dL/dq through q_hat = q / max(||q||, eps): (g - q_hat (q_hat . g)) / ||q||, and
// g / eps under the clamp, where the divisor is a constant and there is no projection term (as torch's autograd has it)
__device__ __forceinline__ float4 act_normalize_backward(float4 q_hat, float norm, float4 dq) {
  if (norm < 1e-12f) return make_float4(dq.x / 1e-12f, dq.y / 1e-12f, dq.z / 1e-12f, dq.w / 1e-12f);
  const float dotg = (q_hat.x * dq.x + q_hat.y * dq.y) + (q_hat.z * dq.z + q_hat.w * dq.w);
  const float dn = fmaxf(norm, 1e-12f);
  return make_float4((dq.x - q_hat.x * dotg) / dn, (dq.y - q_hat.y * dotg) / dn, (dq.z - q_hat.z * dotg) / dn,
                     (dq.w - q_hat.w * dotg) / dn);
}

// The rotation matrix of the quaternion (w,x,y,z), used as given (not re-normalised).
__device__ __forceinline__ void quat_rotation(const float4 q, float R[3][3]) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  R[0][0] = 1.0f - 2.0f * (y * y + z * z);
  R[0][1] = 2.0f * (x * y - r * z);
  R[0][2] = 2.0f * (x * z + r * y);
  R[1][0] = 2.0f * (x * y + r * z);
  R[1][1] = 1.0f - 2.0f * (x * x + z * z);
  R[1][2] = 2.0f * (y * z - r * x);
  R[2][0] = 2.0f * (x * z - r * y);
  R[2][1] = 2.0f * (y * z + r * x);
  R[2][2] = 1.0f - 2.0f * (x * x + y * y);
}
// dL/d(w,x,y,z) from Q[i][j] = dL/dR[i][j] of R = quat_rotation(q).
__device__ __forceinline__ float4 quat_rotation_backward(const float4 q, const float Q[3][3]) {
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  float4 dq;
  dq.x = 2.0f * (-z * Q[0][1] + y * Q[0][2] + z * Q[1][0] - x * Q[1][2] - y * Q[2][0] + x * Q[2][1]);
  dq.y = 2.0f * (y * Q[0][1] + z * Q[0][2] + y * Q[1][0] - 2.0f * x * Q[1][1] - r * Q[1][2] + z * Q[2][0] +
                 r * Q[2][1] - 2.0f * x * Q[2][2]);
  dq.z = 2.0f * (-2.0f * y * Q[0][0] + x * Q[0][1] + r * Q[0][2] + x * Q[1][0] + z * Q[1][2] - r * Q[2][0] +
                 z * Q[2][1] - 2.0f * y * Q[2][2]);
  dq.w = 2.0f * (-2.0f * z * Q[0][0] - r * Q[0][1] + x * Q[0][2] + r * Q[1][0] - 2.0f * z * Q[1][1] +
                 y * Q[1][2] + x * Q[2][0] + y * Q[2][1]);
  return dq;
}

// Sigma = R S S R^T, stored (S00,S01,S02,S11,S12,S22), R = quat_rotation(q).
__device__ __forceinline__ void cov3d_from_scale_rot(const float s3[3], float mod, const float4 q, float cov6[6]) {
  float R[3][3];
  quat_rotation(q, R);
  const float s[3] = {mod * s3[0], mod * s3[1], mod * s3[2]};
  float M[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[k][j] = s[k] * R[j][k];
  auto sig = [&](int i, int j) { return (M[0][i] * M[0][j] + M[1][i] * M[1][j]) + M[2][i] * M[2][j]; };
  cov6[0] = sig(0, 0); cov6[1] = sig(0, 1); cov6[2] = sig(0, 2);
  cov6[3] = sig(1, 1); cov6[4] = sig(1, 2); cov6[5] = sig(2, 2);
}

// The non-zero entries of the perspective Jacobian J at the (clamped) view-space point tc.
__device__ __forceinline__ void ewa_jacobian(const float tc[3], float fx, float fy, float& J00, float& J02, float& J11,
                                             float& J12) {
  const float tx = tc[0], ty = tc[1], tz = tc[2];
  J00 = fx / tz; J02 = -(fx * tx) / (tz * tz);
  J11 = fy / tz; J12 = -(fy * ty) / (tz * tz);
}

// cov2D = (J W) Sigma (J W)^T  ->  (a, b, c) before the 0.3 low-pass.
__device__ __forceinline__ void ewa_cov2d(const float t[3], float fx, float fy, float tanfovx, float tanfovy,
                                          const float cov6[6], const Mat16& V, float abc[3], float T[2][3],
                                          float tclamped[3], bool& clampx, bool& clampy) {
  const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
  const float tz = t[2];
  const float txtz = t[0] / tz, tytz = t[1] / tz;
  const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz;
  const float ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
  clampx = (txtz < -limx) || (txtz > limx);
  clampy = (tytz < -limy) || (tytz > limy);
  tclamped[0] = tx; tclamped[1] = ty; tclamped[2] = tz;
  float J00, J02, J11, J12;
  ewa_jacobian(tclamped, fx, fy, J00, J02, J11, J12);
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // W[r][c] = V.m[4c + r]
    T[0][j] = J00 * V.m[4 * j + 0] + J02 * V.m[4 * j + 2];
    T[1][j] = J11 * V.m[4 * j + 1] + J12 * V.m[4 * j + 2];
  }
  const float S[3][3] = {{cov6[0], cov6[1], cov6[2]}, {cov6[1], cov6[3], cov6[4]}, {cov6[2], cov6[4], cov6[5]}};
  float U[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) U[i][j] = (T[i][0] * S[0][j] + T[i][1] * S[1][j]) + T[i][2] * S[2][j];
  abc[0] = (U[0][0] * T[0][0] + U[0][1] * T[0][1]) + U[0][2] * T[0][2];
  abc[1] = (U[0][0] * T[1][0] + U[0][1] * T[1][1]) + U[0][2] * T[1][2];
  abc[2] = (U[1][0] * T[1][0] + U[1][1] * T[1][1]) + U[1][2] * T[1][2];
}

// ---- backward pieces, shared by the per-Gaussian backward (ggd_preprocess_bwd.hip) and the camera backward (ggd_camera.hip).
// Conventions of the published backward: 1/(det^2 + 1e-7), dL_dconic slot B = half the true d/dB.

// Conic gradient (gA, gB, gC) -> dL/d(a, b, c) of the 2D covariance abc (before the 0.3 dilation).  false: denom^2 overflowed
// (1 / (denom^2 + 1e-7) == 0) and the three are zero.
// AA (ggd_params.antialiasing): the blend saw o_eff = o h, h = sqrt(max(2.5e-5, r)), r = det0 / det1 (before / after the dilation).
// aa_h receives the forward's h, bit for bit; with g_o = dL/do_eff and while the clamp is off the h chain is added:
//   dL/da += k w (c0^2 + w c0 + b^2),  dL/dc += k w (a0^2 + w a0 + b^2),  dL/db += -2 k w b (a0 + c0 + w),  k = g_o o / (2 h det1^2)
template <bool AA>
__device__ __forceinline__ bool cov2d_backward(const float abc[3], float gA, float gB, float gC, float g_o, float o,
                                               float& aa_h, float& dL_da, float& dL_db, float& dL_dc) {
  const float a = abc[0] + 0.3f, b = abc[1], c = abc[2] + 0.3f;
  const float denom = a * c - b * b;
  const float denom2inv = 1.0f / (denom * denom + 0.0000001f);
  float aa_r = 0.0f;
  if constexpr (AA) {   // the forward's h, bit for bit (same fp32 expressions, correctly rounded division and square root)
    aa_r = (abc[0] * abc[2] - abc[1] * abc[1]) / denom;
    aa_h = sqrtf(fmaxf(2.5e-5f, aa_r));
  }
  dL_da = 0.0f; dL_db = 0.0f; dL_dc = 0.0f;
  if (denom2inv == 0.0f) return false;
  dL_da = denom2inv * (-c * c * gA + 2.0f * b * c * gB + (denom - a * c) * gC);
  dL_dc = denom2inv * (-a * a * gC + 2.0f * a * b * gB + (denom - a * c) * gA);
  dL_db = denom2inv * 2.0f * (b * c * gA - (denom + 2.0f * b * b) * gB + a * b * gC);
  // AA: the h chain joins here, so that dL_dcov3D and dT carry it.  Behind the guard: denom2inv == 0 means denom^2 overflowed,
  // where k (1 / det1^2) is 0 as well
  if constexpr (AA) {
    if (aa_r > 2.5e-5f) {
      const float x = abc[0], z = abc[1], y = abc[2], w = 0.3f;
      const float k = g_o * o / (2.0f * aa_h * denom * denom);
      dL_da += k * w * (y * y + w * y + z * z);
      dL_dc += k * w * (x * x + w * x + z * z);
      dL_db += -2.0f * k * w * z * (x + y + w);
    }
  }
  return true;
}

// dL/dT of the EWA matrix T = J W from dL/d(a, b, c):  abc = T Sigma T^T.
__device__ __forceinline__ void ewa_dT(const float T[2][3], const float cov6[6], float dL_da, float dL_db, float dL_dc,
                                       float dT[2][3]) {
  const float S[3][3] = {{cov6[0], cov6[1], cov6[2]}, {cov6[1], cov6[3], cov6[4]}, {cov6[2], cov6[4], cov6[5]}};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float s0 = T[0][0] * S[0][j] + T[0][1] * S[1][j] + T[0][2] * S[2][j];
    const float s1 = T[1][0] * S[0][j] + T[1][1] * S[1][j] + T[1][2] * S[2][j];
    dT[0][j] = 2.0f * s0 * dL_da + s1 * dL_db;
    dT[1][j] = 2.0f * s1 * dL_dc + s0 * dL_db;
  }
}

// dL/dt of the view-space point t = V (p, 1) through J in T = J W, at the clamped point tc.  clampx / clampy: the forward clamped
// x / y, which the published backward treats as independent of z (their gradient is dropped, not rerouted).
__device__ __forceinline__ void ewa_dt(const Mat16& V, const float dT[2][3], float fx, float fy, const float tc[3], bool clampx,
                                       bool clampy, float dt[3]) {
  const float x_grad_mul = clampx ? 0.0f : 1.0f, y_grad_mul = clampy ? 0.0f : 1.0f;
  // W[r][c] = V.m[4c + r]
  const float dJ00 = V.m[0] * dT[0][0] + V.m[4] * dT[0][1] + V.m[8] * dT[0][2];
  const float dJ02 = V.m[2] * dT[0][0] + V.m[6] * dT[0][1] + V.m[10] * dT[0][2];
  const float dJ11 = V.m[1] * dT[1][0] + V.m[5] * dT[1][1] + V.m[9] * dT[1][2];
  const float dJ12 = V.m[2] * dT[1][0] + V.m[6] * dT[1][1] + V.m[10] * dT[1][2];
  const float tz = 1.0f / tc[2], tz2 = tz * tz, tz3 = tz2 * tz;
  dt[0] = x_grad_mul * -fx * tz2 * dJ02;
  dt[1] = y_grad_mul * -fy * tz2 * dJ12;
  dt[2] = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.0f * fx * tc[0]) * tz3 * dJ02 + (2.0f * fy * tc[1]) * tz3 * dJ12;
}

// The perspective divide of h = PV (p, 1):  m_w = 1 / (h3 + 1e-7), mul1 = h0 m_w^2, mul2 = h1 m_w^2.  With (g0, g1) the gradient of
// the screen position, dL/dh = (m_w g0, m_w g1, -, -(mul1 g0 + mul2 g1)).
__device__ __forceinline__ void divide_terms(const Mat16& PV, const float p[3], float& m_w, float& mul1, float& mul2) {
  const float h0 = PV.m[0] * p[0] + PV.m[4] * p[1] + PV.m[8] * p[2] + PV.m[12];
  const float h1 = PV.m[1] * p[0] + PV.m[5] * p[1] + PV.m[9] * p[2] + PV.m[13];
  const float h3 = PV.m[3] * p[0] + PV.m[7] * p[1] + PV.m[11] * p[2] + PV.m[15];
  m_w = 1.0f / (h3 + 0.0000001f);
  mul1 = h0 * m_w * m_w; mul2 = h1 * m_w * m_w;
}

// d (colour channel c, before the clamp) / d (x, y, z), the unit view direction; sh: the Gaussian's [M][3] coefficients.
__device__ __forceinline__ void sh_dir_grad(int deg, const float* sh, int c, float x, float y, float z, float& dx, float& dy,
                                            float& dz) {
#define SHK(k) sh[(k) * 3 + c]
  dx = 0.0f; dy = 0.0f; dz = 0.0f;
  if (deg > 0) {
    dx = -SH_C1 * SHK(3); dy = -SH_C1 * SHK(1); dz = SH_C1 * SHK(2);
    if (deg > 1) {
      dx += SH_C2[0] * y * SHK(4) + SH_C2[2] * 2.0f * -x * SHK(6) + SH_C2[3] * z * SHK(7) + SH_C2[4] * 2.0f * x * SHK(8);
      dy += SH_C2[0] * x * SHK(4) + SH_C2[1] * z * SHK(5) + SH_C2[2] * 2.0f * -y * SHK(6) + SH_C2[4] * 2.0f * -y * SHK(8);
      dz += SH_C2[1] * y * SHK(5) + SH_C2[2] * 4.0f * z * SHK(6) + SH_C2[3] * x * SHK(7);
      if (deg > 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        dx += SH_C3[0] * SHK(9) * 6.0f * xy + SH_C3[1] * SHK(10) * yz + SH_C3[2] * SHK(11) * -2.0f * xy +
              SH_C3[3] * SHK(12) * -6.0f * xz + SH_C3[4] * SHK(13) * (4.0f * zz - 3.0f * xx - yy) +
              SH_C3[5] * SHK(14) * 2.0f * xz + SH_C3[6] * SHK(15) * 3.0f * (xx - yy);
        dy += SH_C3[0] * SHK(9) * 3.0f * (xx - yy) + SH_C3[1] * SHK(10) * xz +
              SH_C3[2] * SHK(11) * (4.0f * zz - xx - 3.0f * yy) + SH_C3[3] * SHK(12) * -6.0f * yz +
              SH_C3[4] * SHK(13) * -2.0f * xy + SH_C3[5] * SHK(14) * -2.0f * yz + SH_C3[6] * SHK(15) * -6.0f * xy;
        dz += SH_C3[1] * SHK(10) * xy + SH_C3[2] * SHK(11) * 8.0f * yz + SH_C3[3] * SHK(12) * 3.0f * (2.0f * zz - xx - yy) +
              SH_C3[4] * SHK(13) * 8.0f * xz + SH_C3[5] * SHK(14) * (xx - yy);
      }
    }
  }
#undef SHK
}

// dL/dv of v = p - campos from dL/d(v / |v|) = ddir: what the SH colour adds to dL/dmean, and, negated, to dL/dcampos.
__device__ __forceinline__ void dir_to_point(const float v[3], const float ddir[3], float out[3]) {
  const float v0 = v[0], v1 = v[1], v2 = v[2];
  const float sum2 = v0 * v0 + v1 * v1 + v2 * v2;
  const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
  out[0] = ((sum2 - v0 * v0) * ddir[0] - v1 * v0 * ddir[1] - v2 * v0 * ddir[2]) * invsum32;
  out[1] = (-v0 * v1 * ddir[0] + (sum2 - v1 * v1) * ddir[1] - v2 * v1 * ddir[2]) * invsum32;
  out[2] = (-v0 * v2 * ddir[0] - v1 * v2 * ddir[1] + (sum2 - v2 * v2) * ddir[2]) * invsum32;
}

__device__ __forceinline__ void sh_to_rgb(int deg, const float* __restrict__ sh, const float p[3],
                                          const float campos[3], float rgb[3], uint32_t& clamp_bits) {
  float dx = p[0] - campos[0], dy = p[1] - campos[1], dz = p[2] - campos[2];
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  const float x = dx / len, y = dy / len, z = dz / len;
  clamp_bits = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#define SHK(k) sh[(k) * 3 + c]
    float res = SH_C0 * SHK(0);
    if (deg > 0) {
      res = res - SH_C1 * y * SHK(1) + SH_C1 * z * SHK(2) - SH_C1 * x * SHK(3);
      if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        res = res + SH_C2[0] * xy * SHK(4) + SH_C2[1] * yz * SHK(5) + SH_C2[2] * (2.0f * zz - xx - yy) * SHK(6) +
              SH_C2[3] * xz * SHK(7) + SH_C2[4] * (xx - yy) * SHK(8);
        if (deg > 2) {
          res = res + SH_C3[0] * y * (3.0f * xx - yy) * SHK(9) + SH_C3[1] * xy * z * SHK(10) +
                SH_C3[2] * y * (4.0f * zz - xx - yy) * SHK(11) +
                SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * SHK(12) +
                SH_C3[4] * x * (4.0f * zz - xx - yy) * SHK(13) + SH_C3[5] * z * (xx - yy) * SHK(14) +
                SH_C3[6] * x * (xx - 3.0f * yy) * SHK(15);
        }
      }
    }
#undef SHK
    res = res + 0.5f;
    if (res < 0.0f) clamp_bits |= (1u << c);
    rgb[c] = fmaxf(res, 0.0f);
  }
}


}  // namespace ggdm
