// ggd_preprocess_bwd.hip -- stage a11: per-Gaussian backward (conic -> cov2D -> cov3D / view point; screen
// position through the perspective divide; colour -> SH (+ view direction); cov3D -> scale, quaternion).
//
// Replaces computeCov2D-backward + preprocess-backward inside `_C.rasterize_gaussians_backward`, which the
// reference reaches through autograd from main/train_pano2gaussian_decoder.py:263 (loss.backward()).  Algorithm:
// SURVEY.md section 9.6.  One lane per Gaussian, fused into ONE streaming pass (upstream runs two kernels and
// round-trips dL_dcov3D through memory when scales/rotations are given); cov3D is recomputed from scale/rotation
// instead of being stored by the forward pass (saves 24 B/Gaussian written + read).
// Conventions kept from the published algorithm because they change values beyond the 1e-5 tolerance otherwise:
// 1/(det^2 + 1e-7) in the conic inverse, dL_dconic slot 1 = half the true d/dB, and the clamped view-space x,y
// treated as independent of z.
#include "ggd_math.h"

namespace {
using namespace ggdm;

// The per-Gaussian work of the kernels below.  dsh_stage: where this Gaussian's 3 M SH gradients go instead of
// dL_dsh[i] (the staged kernel's LDS row), or nullptr.
// SHVEC: the Gaussian's SH row is read with dwordx4 loads into registers (see preprocess_kernel); DREG: its gradients are
// collected in registers too and leave as 3 M / 4 dwordx4 stores.  AUX (depth / alpha extension): the accumulator record's
// slot GGD_ACC_DEPTH holds dL/dz of the view-space depth z = view row 2 . (p, 1), added to dL/dmean (z is not clamped).
// AA (anti-aliasing, ggd_params.antialiasing): the blend saw o_eff = o h, h = sqrt(max(2.5e-5, r)), r = det0 / det1 with
// det0 = x y - z^2 and det1 = (x + w)(y + w) - z^2 the determinants of the 2D covariance (x, z, y) = abc before / after the
// w = 0.3 dilation.  With g = dL/do_eff (acc0.w): dL/do = g h, and while the clamp is off dL/dr = g o / (2 h) adds
//   dL/dx += k w (y^2 + w y + z^2),  dL/dy += k w (x^2 + w x + z^2),  dL/dz += -2 k w z (x + y + w),  k = g o / (2 h det1^2)
// to the conic's dL/da, dL/dc, dL/db before they are taken on to cov3D and the view-space point
// ABS (absgrad extension): dL_dmean2D_abs[i] = (accumulator slots GGD_ACC_ABS, GGD_ACC_ABS + 1, 0) -- the blend's sums of the
// per-pixel absolute screen-space gradients, already scaled -- and zeros for a culled Gaussian; nothing else changes
template <bool SHVEC, bool DREG = false, bool AUX = false, bool AA = false, bool ABS = false>
__device__ __forceinline__ void preprocess_backward_body(
    int i, float* dsh_stage,
    int P, int M, int deg, int W, int H, float tanfovx, float tanfovy, float mod, int raw,
    const float* __restrict__ opacities_raw, float* __restrict__ dL_dopacity,
    const float* __restrict__ view, const float* __restrict__ proj, const float* __restrict__ campos_p,
    const float* __restrict__ means3D, const float* __restrict__ shs, const float* __restrict__ colors_precomp,
    const float* __restrict__ scales, const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
    const int32_t* __restrict__ radii, const uint8_t* __restrict__ clamped,
    const float* __restrict__ grad_acc, float* __restrict__ dL_dmean2D, float* __restrict__ dL_dcolors,
    float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dcov3D, float* __restrict__ dL_dsh,
    float* __restrict__ dL_dscales, float* __restrict__ dL_drots, float* __restrict__ dL_dmean2D_abs) {
  const size_t ii = (size_t)i;
  if (radii[i] <= 0) {  // culled: every gradient of this Gaussian is zero (the caller does not pre-fill the arrays)
    dL_dmean2D[3 * ii] = 0.0f; dL_dmean2D[3 * ii + 1] = 0.0f; dL_dmean2D[3 * ii + 2] = 0.0f;
    if constexpr (ABS) { dL_dmean2D_abs[3 * ii] = 0.0f; dL_dmean2D_abs[3 * ii + 1] = 0.0f; dL_dmean2D_abs[3 * ii + 2] = 0.0f; }
    dL_dcolors[3 * ii] = 0.0f; dL_dcolors[3 * ii + 1] = 0.0f; dL_dcolors[3 * ii + 2] = 0.0f;
    dL_dopacity[i] = 0.0f;
    dL_dmeans3D[3 * ii] = 0.0f; dL_dmeans3D[3 * ii + 1] = 0.0f; dL_dmeans3D[3 * ii + 2] = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) dL_dcov3D[6 * ii + k] = 0.0f;
    if (!colors_precomp) {
      if (DREG) {
        float4* z4 = reinterpret_cast<float4*>(dL_dsh + ii * M * 3);
        for (int qd = 0; qd < ((3 * M) >> 2); ++qd) z4[qd] = make_float4(0, 0, 0, 0);
      } else {
        float* z = dsh_stage ? dsh_stage : dL_dsh + ii * M * 3;
        for (int k = 0; k < 3 * M; ++k) z[k] = 0.0f;
      }
    }
    if (!cov3D_precomp) {
      dL_dscales[3 * ii] = 0.0f; dL_dscales[3 * ii + 1] = 0.0f; dL_dscales[3 * ii + 2] = 0.0f;
      reinterpret_cast<float4*>(dL_drots)[i] = make_float4(0, 0, 0, 0);
    }
    return;
  }
  const float4 acc0 = reinterpret_cast<const float4*>(grad_acc)[3 * ii];      // conic A, B, C | opacity
  const float4 acc1 = reinterpret_cast<const float4*>(grad_acc)[3 * ii + 1];  // mean2D x, y | colour r, g
  const float4 acc2 = reinterpret_cast<const float4*>(grad_acc)[3 * ii + 2];  // colour b | depth | abs mean2D x, y
  const float gcol3[3] = {acc1.z, acc1.w, acc2.x};
  dL_dmean2D[3 * ii] = acc1.x; dL_dmean2D[3 * ii + 1] = acc1.y; dL_dmean2D[3 * ii + 2] = 0.0f;
  if constexpr (ABS) {
    static_assert(GGD_ACC_ABS == 10, "absolute mean gradients are read from acc2.z, acc2.w");
    dL_dmean2D_abs[3 * ii] = acc2.z; dL_dmean2D_abs[3 * ii + 1] = acc2.w; dL_dmean2D_abs[3 * ii + 2] = 0.0f;
  }
  dL_dcolors[3 * ii] = gcol3[0]; dL_dcolors[3 * ii + 1] = gcol3[1]; dL_dcolors[3 * ii + 2] = gcol3[2];
  const Mat16 V = load_mat(view);
  const Mat16 PV = load_mat(proj);
  const float p[3] = {means3D[3 * ii], means3D[3 * ii + 1], means3D[3 * ii + 2]};

  float c6[6];
  float4 q = make_float4(0, 0, 0, 0), q_raw = make_float4(0, 0, 0, 0);
  float q_norm = 1.0f;
  float s3[3] = {0, 0, 0};
  if (cov3D_precomp) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = cov3D_precomp[6 * ii + k];
  } else {
    s3[0] = scales[3 * ii]; s3[1] = scales[3 * ii + 1]; s3[2] = scales[3 * ii + 2];
    q = reinterpret_cast<const float4*>(rotations)[i];
    if (raw) {
      q_raw = q;
      s3[0] = expf(s3[0]); s3[1] = expf(s3[1]); s3[2] = expf(s3[2]);
      q = act_normalize(q, q_norm);
    }
    cov3d_from_scale_rot(s3, mod, q, c6);
  }

  float dmean[3];
  float dc[6] = {0, 0, 0, 0, 0, 0};
  float aa_o = 0.0f, aa_h = 1.0f;   // AA: the opacity o (activated) and h of the forward
  if constexpr (AA) aa_o = raw ? act_sigmoid(opacities_raw[i]) : opacities_raw[i];
  // (1) conic -> cov2D -> cov3D, view-space point
  {
    float t[3];
    t[0] = V.m[0] * p[0] + V.m[4] * p[1] + V.m[8] * p[2] + V.m[12];
    t[1] = V.m[1] * p[0] + V.m[5] * p[1] + V.m[9] * p[2] + V.m[13];
    t[2] = V.m[2] * p[0] + V.m[6] * p[1] + V.m[10] * p[2] + V.m[14];
    const float fx = (float)W / (2.0f * tanfovx), fy = (float)H / (2.0f * tanfovy);
    float abc[3], T[2][3], tc[3];
    bool clx, cly;
    ewa_cov2d(t, fx, fy, tanfovx, tanfovy, c6, V, abc, T, tc, clx, cly);
    float dL_da, dL_db, dL_dc;
    if (cov2d_backward<AA>(abc, acc0.x, acc0.y, acc0.z, acc0.w, aa_o, aa_h, dL_da, dL_db, dL_dc)) {
      dc[0] = T[0][0] * T[0][0] * dL_da + T[0][0] * T[1][0] * dL_db + T[1][0] * T[1][0] * dL_dc;
      dc[3] = T[0][1] * T[0][1] * dL_da + T[0][1] * T[1][1] * dL_db + T[1][1] * T[1][1] * dL_dc;
      dc[5] = T[0][2] * T[0][2] * dL_da + T[0][2] * T[1][2] * dL_db + T[1][2] * T[1][2] * dL_dc;
      dc[1] = 2.0f * T[0][0] * T[0][1] * dL_da + (T[0][0] * T[1][1] + T[0][1] * T[1][0]) * dL_db +
              2.0f * T[1][0] * T[1][1] * dL_dc;
      dc[2] = 2.0f * T[0][0] * T[0][2] * dL_da + (T[0][0] * T[1][2] + T[0][2] * T[1][0]) * dL_db +
              2.0f * T[1][0] * T[1][2] * dL_dc;
      dc[4] = 2.0f * T[0][2] * T[0][1] * dL_da + (T[0][1] * T[1][2] + T[0][2] * T[1][1]) * dL_db +
              2.0f * T[1][1] * T[1][2] * dL_dc;
    }
    float dT[2][3], dt[3];
    ewa_dT(T, c6, dL_da, dL_db, dL_dc, dT);
    ewa_dt(V, dT, fx, fy, tc, clx, cly, dt);
    const float dtx = dt[0], dty = dt[1], dtz = dt[2];
    dmean[0] = V.m[0] * dtx + V.m[1] * dty + V.m[2] * dtz;
    dmean[1] = V.m[4] * dtx + V.m[5] * dty + V.m[6] * dtz;
    dmean[2] = V.m[8] * dtx + V.m[9] * dty + V.m[10] * dtz;
  }
  // (2) screen position through the perspective divide
  {
    float m_w, mul1, mul2;
    divide_terms(PV, p, m_w, mul1, mul2);
    const float g0 = acc1.x, g1 = acc1.y;
    dmean[0] += (PV.m[0] * m_w - PV.m[3] * mul1) * g0 + (PV.m[1] * m_w - PV.m[3] * mul2) * g1;
    dmean[1] += (PV.m[4] * m_w - PV.m[7] * mul1) * g0 + (PV.m[5] * m_w - PV.m[7] * mul2) * g1;
    dmean[2] += (PV.m[8] * m_w - PV.m[11] * mul1) * g0 + (PV.m[9] * m_w - PV.m[11] * mul2) * g1;
  }
  // (3) colour -> SH coefficients (+ position through the view direction when deg > 0)
  if (!colors_precomp) {
    float shr[SHVEC ? 48 : 1];
    const float* sh;
    if constexpr (SHVEC) {
      const float4* src = reinterpret_cast<const float4*>(shs + ii * M * 3);
      const int nq = deg > 0 ? (3 * M) >> 2 : 0;   // (degree 0 reads no coefficient)
#pragma unroll
      for (int qd = 0; qd < 12; ++qd) {
        float4 v = make_float4(0, 0, 0, 0);
        if (qd < nq) v = src[qd];
        shr[4 * qd] = v.x; shr[4 * qd + 1] = v.y; shr[4 * qd + 2] = v.z; shr[4 * qd + 3] = v.w;
      }
      sh = shr;
    } else {
      shr[0] = 0.0f;
      sh = shs + ii * M * 3;
    }
    // SHVEC without a staging row: the gradients are collected in registers and leave as 3 M / 4 dwordx4 stores
    float dshr[DREG ? 48 : 1];
    float* dsh;
    if constexpr (DREG) {
#pragma unroll
      for (int k = 0; k < 48; ++k) dshr[k] = 0.0f;
      dsh = dshr;
    } else {
      dshr[0] = 0.0f;
      dsh = dsh_stage ? dsh_stage : dL_dsh + ii * M * 3;
    }
    const uint32_t cl = clamped[i];
    const float v0 = p[0] - campos_p[0], v1 = p[1] - campos_p[1], v2 = p[2] - campos_p[2];
    const float len = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
    const float x = v0 / len, y = v1 / len, z = v2 / len;
    float ddir[3] = {0.0f, 0.0f, 0.0f};
    // coefficients above the active degree (M > (deg+1)^2, e.g. max_sh_degree 3 with active degree 1) take no part
    // in the colour: their gradient is zero and is written here (the caller does not pre-fill the arrays)
    if constexpr (!DREG)
      for (int k = 3 * (deg + 1) * (deg + 1); k < 3 * M; ++k) dsh[k] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gcol = ((cl >> c) & 1u) ? 0.0f : gcol3[c];
#define DSH(k) dsh[(k) * 3 + c]
      float dx, dy, dz;
      sh_dir_grad(deg, sh, c, x, y, z, dx, dy, dz);
      DSH(0) = SH_C0 * gcol;
      if (deg > 0) {
        DSH(1) = -SH_C1 * y * gcol; DSH(2) = SH_C1 * z * gcol; DSH(3) = -SH_C1 * x * gcol;
        if (deg > 1) {
          const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
          DSH(4) = SH_C2[0] * xy * gcol; DSH(5) = SH_C2[1] * yz * gcol;
          DSH(6) = SH_C2[2] * (2.0f * zz - xx - yy) * gcol;
          DSH(7) = SH_C2[3] * xz * gcol; DSH(8) = SH_C2[4] * (xx - yy) * gcol;
          if (deg > 2) {
            DSH(9) = SH_C3[0] * y * (3.0f * xx - yy) * gcol;
            DSH(10) = SH_C3[1] * xy * z * gcol;
            DSH(11) = SH_C3[2] * y * (4.0f * zz - xx - yy) * gcol;
            DSH(12) = SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * gcol;
            DSH(13) = SH_C3[4] * x * (4.0f * zz - xx - yy) * gcol;
            DSH(14) = SH_C3[5] * z * (xx - yy) * gcol;
            DSH(15) = SH_C3[6] * x * (xx - 3.0f * yy) * gcol;
          }
        }
      }
#undef DSH
      ddir[0] += dx * gcol; ddir[1] += dy * gcol; ddir[2] += dz * gcol;
    }
    if constexpr (DREG) {
      {
        float4* d4 = reinterpret_cast<float4*>(dL_dsh + ii * M * 3);
        const int nq = (3 * M) >> 2;
#pragma unroll
        for (int qd = 0; qd < 12; ++qd)
          if (qd < nq) d4[qd] = make_float4(dshr[4 * qd], dshr[4 * qd + 1], dshr[4 * qd + 2], dshr[4 * qd + 3]);
      }
    }
    if (deg > 0) {
      const float v[3] = {v0, v1, v2};
      float dv[3];
      dir_to_point(v, ddir, dv);
      dmean[0] += dv[0]; dmean[1] += dv[1]; dmean[2] += dv[2];
    }
  }
  if constexpr (AUX) {
    static_assert(GGD_ACC_DEPTH == 9, "depth gradient is read from acc2.y");
    const float gz = acc2.y;
    dmean[0] += V.m[2] * gz; dmean[1] += V.m[6] * gz; dmean[2] += V.m[10] * gz;
  }
  dL_dmeans3D[3 * ii] = dmean[0]; dL_dmeans3D[3 * ii + 1] = dmean[1]; dL_dmeans3D[3 * ii + 2] = dmean[2];
#pragma unroll
  for (int k = 0; k < 6; ++k) dL_dcov3D[6 * ii + k] = dc[k];

  // (4) cov3D -> scale, quaternion
  if (!cov3D_precomp) {
    float R[3][3];
    quat_rotation(q, R);
    const float s[3] = {mod * s3[0], mod * s3[1], mod * s3[2]};
    float Mm[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) Mm[k][j] = s[k] * R[j][k];
    const float Gs[3][3] = {{dc[0], 0.5f * dc[1], 0.5f * dc[2]},
                            {0.5f * dc[1], dc[3], 0.5f * dc[4]},
                            {0.5f * dc[2], 0.5f * dc[4], dc[5]}};
    float dM[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        dM[k][j] = 2.0f * (Mm[k][0] * Gs[0][j] + Mm[k][1] * Gs[1][j] + Mm[k][2] * Gs[2][j]);
    float Q[3][3];
    float dscale[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dscale[k] = mod * (R[0][k] * dM[k][0] + R[1][k] * dM[k][1] + R[2][k] * dM[k][2]);
#pragma unroll
      for (int j = 0; j < 3; ++j) Q[j][k] = dM[k][j] * s[k];
    }
    if (raw) {  // d exp(x) = exp(x)
      dscale[0] *= s3[0]; dscale[1] *= s3[1]; dscale[2] *= s3[2];
    }
    dL_dscales[3 * ii] = dscale[0]; dL_dscales[3 * ii + 1] = dscale[1]; dL_dscales[3 * ii + 2] = dscale[2];
    float4 dq = quat_rotation_backward(q, Q);
    if (raw) {
      dq = act_normalize_backward(q, q_norm, dq);
      (void)q_raw;
    }
    reinterpret_cast<float4*>(dL_drots)[i] = dq;
  }
  const float g_op = AA ? acc0.w * aa_h : acc0.w;   // AA: dL/do = dL/do_eff h
  if (raw) {  // sigmoid'(x) = s (1 - s) applied to the blend's dL/d(opacity)
    const float sg = act_sigmoid(opacities_raw[i]);
    dL_dopacity[i] = g_op * (sg * (1.0f - sg));
  } else {
    dL_dopacity[i] = g_op;
  }
}

#define GGD_PPB_PARAMS                                                                                                  \
    int P, int M, int deg, int W, int H, float tanfovx, float tanfovy, float mod, int raw,                              \
    const float* __restrict__ opacities_raw, float* __restrict__ dL_dopacity, const float* __restrict__ view,           \
    const float* __restrict__ proj, const float* __restrict__ campos_p, const float* __restrict__ means3D,              \
    const float* __restrict__ shs, const float* __restrict__ colors_precomp, const float* __restrict__ scales,          \
    const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, const int32_t* __restrict__ radii,    \
    const uint8_t* __restrict__ clamped, const float* __restrict__ grad_acc, float* __restrict__ dL_dmean2D,            \
    float* __restrict__ dL_dcolors, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dcov3D,                     \
    float* __restrict__ dL_dsh, float* __restrict__ dL_dscales, float* __restrict__ dL_drots
#define GGD_PPB_ARGS                                                                                                    \
    P, M, deg, W, H, tanfovx, tanfovy, mod, raw, opacities_raw, dL_dopacity, view, proj, campos_p, means3D, shs,        \
    colors_precomp, scales, rotations, cov3D_precomp, radii, clamped, grad_acc, dL_dmean2D, dL_dcolors, dL_dmeans3D,    \
    dL_dcov3D, dL_dsh, dL_dscales, dL_drots

// The three forms of the kernel.  AA: the anti-aliasing h chain (ggd_params.antialiasing); AUX: the depth term of the
// depth / alpha extension (ggd_backward_aux).  Both off: the plain backward.
// The absgrad extension (ggd_backward_abs) has kernels of its own, preprocess_abs_backward{,_vec,_staged}_kernel: the same
// bodies with ABS on and one more argument, dL_dmean2D_abs.  The kernels below keep their names, arguments and code.
template <bool AA = false, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_backward_kernel(GGD_PPB_PARAMS) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  preprocess_backward_body<false, false, AUX, AA>(i, nullptr, GGD_PPB_ARGS, nullptr);
}

template <bool AA = false, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_abs_backward_kernel(GGD_PPB_PARAMS, float* __restrict__ dL_dmean2D_abs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  preprocess_backward_body<false, false, AUX, AA, true>(i, nullptr, GGD_PPB_ARGS, dL_dmean2D_abs);
}

template <bool AA = false, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_backward_vec_kernel(GGD_PPB_PARAMS) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  preprocess_backward_body<true, true, AUX, AA>(i, nullptr, GGD_PPB_ARGS, nullptr);
}

template <bool AA = false, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_abs_backward_vec_kernel(GGD_PPB_PARAMS, float* __restrict__ dL_dmean2D_abs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  preprocess_backward_body<true, true, AUX, AA, true>(i, nullptr, GGD_PPB_ARGS, dL_dmean2D_abs);
}

// SH degree > 0 (M > 1 coefficients per channel): a Gaussian's 3 M gradients are 12 M bytes apart from its neighbour's, so
// written by their owner lane they leave the wave as 3 M store instructions of 64 lone words each (1 M Gaussians, M = 16:
// 494 us for this kernel against 88 us at M = 1).  Here every lane parks its row in LDS and the wave writes its 64 rows --
// one contiguous 768 M-byte span of dL_dsh -- with lane-consecutive (16-byte where 3 M allows) stores.  (1 M Gaussians,
// M = 16: 247 -> 146 us; preprocess_backward_vec_kernel above does as well without LDS where the rows allow dwordx4.)
// (the write-out of the staged rows, after the wave's lanes have parked them)
__device__ __forceinline__ void preprocess_backward_flush_rows(const float* s_dsh, float* __restrict__ dL_dsh, int P, int M) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rl = 3 * M, rowlen = rl + 1;
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  const int i0 = blockIdx.x * 256 + wv * 64;
  const int nrows = min(64, P - i0);
  if (nrows <= 0) return;
  const float* rows = s_dsh + (size_t)wv * 64 * rowlen;
  float* dst = dL_dsh + (size_t)i0 * rl;
  const int total = nrows * rl;
  if ((rl & 3) == 0) {
    for (int e = 4 * lane; e < total; e += 256) {
      const int r = e / rl, k = e - r * rl;
      const float* src = rows + r * rowlen + k;
      *reinterpret_cast<float4*>(dst + e) = make_float4(src[0], src[1], src[2], src[3]);
    }
  } else {
    for (int e = lane; e < total; e += 64) {
      const int r = e / rl, k = e - r * rl;
      dst[e] = rows[r * rowlen + k];
    }
  }
}

template <bool SHVEC, bool AA = false, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_backward_staged_kernel(GGD_PPB_PARAMS) {
  extern __shared__ float s_dsh[];   // [256][3 M + 1]
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < P) preprocess_backward_body<SHVEC, false, AUX, AA>(i, s_dsh + (size_t)threadIdx.x * (3 * M + 1), GGD_PPB_ARGS, nullptr);
  preprocess_backward_flush_rows(s_dsh, dL_dsh, P, M);
}

template <bool SHVEC, bool AA = false, bool AUX = false>
__global__ __launch_bounds__(256) void preprocess_abs_backward_staged_kernel(GGD_PPB_PARAMS,
                                                                             float* __restrict__ dL_dmean2D_abs) {
  extern __shared__ float s_dsh[];   // [256][3 M + 1]
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < P)
    preprocess_backward_body<SHVEC, false, AUX, AA, true>(i, s_dsh + (size_t)threadIdx.x * (3 * M + 1), GGD_PPB_ARGS, dL_dmean2D_abs);
  preprocess_backward_flush_rows(s_dsh, dL_dsh, P, M);
}

}  // namespace

int ggd_launch_preprocess_backward(ggd_ctx* ctx, hipStream_t s, const ggd_params& prm, const ggd_inputs& in,
                                   const int32_t* radii, const uint8_t* clamped, const float* grad_acc, const ggd_grads& out,
                                   bool aux) {
  if (prm.P == 0) return GGD_OK;
  // the staged form whenever there is more than the band-0 coefficient per channel (and room: 256 rows of 3 M + 1 floats)
  const bool staged = !in.colors_precomp && prm.M > 1 && (size_t)256 * (3 * prm.M + 1) * sizeof(float) <= 64 * 1024;
  // rows that are a multiple of 16 bytes (M = 4, 8, 12, 16): read and written from registers with dwordx4 accesses (145 us
  // at M = 16, 1 M Gaussians; the LDS-staged form measures 152 with the same loads and is kept for the other M)
  const bool shvec = staged && prm.M <= 16 && ((3 * prm.M) & 3) == 0;
  // the feature flags (h chain, depth term, absolute gradients) pick the instance, the SH layout picks the form
  const size_t lds = (staged && !shvec) ? (size_t)256 * (3 * prm.M + 1) * sizeof(float) : 0;
  ggd_dispatch<2>(prm.antialiasing != 0, [&](auto aa) {
    ggd_dispatch<2>(aux, [&](auto ax) {
      constexpr bool AA = decltype(aa)::value != 0, AUX = decltype(ax)::value != 0;
      if (out.dL_dmeans2D_abs) {   // the absgrad kernels: one more argument
        const auto kernel = shvec ? preprocess_abs_backward_vec_kernel<AA, AUX>
                          : staged ? preprocess_abs_backward_staged_kernel<false, AA, AUX> : preprocess_abs_backward_kernel<AA, AUX>;
        hipLaunchKernelGGL(kernel, dim3((prm.P + 255) / 256), dim3(256), lds, s, prm.P, prm.M, prm.sh_degree, prm.width,
                           prm.height, prm.tanfovx, prm.tanfovy, prm.scale_modifier, prm.raw_attributes, in.opacities,
                           out.dL_dopacity, prm.viewmatrix, prm.projmatrix, prm.campos, in.means3D, in.shs, in.colors_precomp,
                           in.scales, in.rotations, in.cov3D_precomp, radii, clamped, grad_acc, out.dL_dmeans2D, out.dL_dcolors,
                           out.dL_dmeans3D, out.dL_dcov3D, out.dL_dsh, out.dL_dscales, out.dL_drots, out.dL_dmeans2D_abs);
        return;
      }
      const auto kernel = shvec ? preprocess_backward_vec_kernel<AA, AUX>
                        : staged ? preprocess_backward_staged_kernel<false, AA, AUX> : preprocess_backward_kernel<AA, AUX>;
      hipLaunchKernelGGL(kernel, dim3((prm.P + 255) / 256), dim3(256), lds, s, prm.P, prm.M, prm.sh_degree, prm.width,
                         prm.height, prm.tanfovx, prm.tanfovy, prm.scale_modifier, prm.raw_attributes, in.opacities,
                         out.dL_dopacity, prm.viewmatrix, prm.projmatrix, prm.campos, in.means3D, in.shs, in.colors_precomp,
                         in.scales, in.rotations, in.cov3D_precomp, radii, clamped, grad_acc, out.dL_dmeans2D, out.dL_dcolors,
                         out.dL_dmeans3D, out.dL_dcov3D, out.dL_dsh, out.dL_dscales, out.dL_drots);
    });
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
