// ggd_normals.hip -- per-Gaussian view-space normals and their gradient (ggd_gaussian_normals / _backward).
// A splat's normal is its shortest axis, column k = argmin scales of R = quat_rotation(q), taken into view space and turned
// towards the camera.  One thread per Gaussian, streaming: no atomics, no scratch, no LDS, no host wait.  The argmin and the
// facing sign are decisions on the inputs (no gradient); both kernels evaluate them through the same function, so the backward
// differentiates exactly the branch the forward took.
#include "ggd_common.h"
#include "ggd_math.h"

namespace {

using namespace ggdm;

struct NormalRow {
  float4 q;      // the quaternion R is built from (normalised when raw)
  float q_norm;  // raw: the norm act_normalize divided by
  int k;         // argmin of the scales, ties to the lowest index
  float sign;    // -1 where the view-space axis points away from the camera
  float n[3];    // the normal
};

__device__ __forceinline__ NormalRow normal_row(int i, const float* __restrict__ rotations, const float* __restrict__ scales,
                                                const float* __restrict__ means3D, const Mat16& V, int raw) {
  NormalRow r;
  r.q = reinterpret_cast<const float4*>(rotations)[i];
  r.q_norm = 1.0f;
  if (raw) r.q = act_normalize(r.q, r.q_norm);
  const float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];   // raw: log-scales, the same argmin
  r.k = (s1 < s0) ? 1 : 0;
  if (s2 < (r.k ? s1 : s0)) r.k = 2;
  float R[3][3];
  quat_rotation(r.q, R);
  const float nw[3] = {R[0][r.k], R[1][r.k], R[2][r.k]};
  const float p[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
  float nv[3], pv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // row-vector convention: v_view = v . V[:3,:3] (+ V[3,:3]), V[a][c] = m[4a + c]
    nv[c] = (nw[0] * V.m[c] + nw[1] * V.m[4 + c]) + nw[2] * V.m[8 + c];
    pv[c] = ((p[0] * V.m[c] + p[1] * V.m[4 + c]) + p[2] * V.m[8 + c]) + V.m[12 + c];
  }
  const float facing = (nv[0] * pv[0] + nv[1] * pv[1]) + nv[2] * pv[2];
  r.sign = facing > 0.0f ? -1.0f : 1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) r.n[c] = r.sign * nv[c];
  return r;
}

__global__ __launch_bounds__(256) void gaussian_normals_kernel(int P, const float* __restrict__ rotations,
                                                               const float* __restrict__ scales,
                                                               const float* __restrict__ means3D,
                                                               const float* __restrict__ viewmatrix, int raw,
                                                               float* __restrict__ normals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const NormalRow r = normal_row(i, rotations, scales, means3D, load_mat(viewmatrix), raw);
  normals[3 * i] = r.n[0]; normals[3 * i + 1] = r.n[1]; normals[3 * i + 2] = r.n[2];
}

__global__ __launch_bounds__(256) void gaussian_normals_backward_kernel(int P, const float* __restrict__ rotations,
                                                                        const float* __restrict__ scales,
                                                                        const float* __restrict__ means3D,
                                                                        const float* __restrict__ viewmatrix, int raw,
                                                                        const float* __restrict__ dL_dnormals,
                                                                        float* __restrict__ dL_drotations) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const Mat16 V = load_mat(viewmatrix);
  const NormalRow r = normal_row(i, rotations, scales, means3D, V, raw);
  const float gv[3] = {r.sign * dL_dnormals[3 * i], r.sign * dL_dnormals[3 * i + 1], r.sign * dL_dnormals[3 * i + 2]};
  float Q[3][3];   // dL/dR: column k holds V[:3,:3] gv, the other two are zero
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float gw = (V.m[4 * a] * gv[0] + V.m[4 * a + 1] * gv[1]) + V.m[4 * a + 2] * gv[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[a][c] = (c == r.k) ? gw : 0.0f;
  }
  float4 dq = quat_rotation_backward(r.q, Q);
  if (raw) dq = act_normalize_backward(r.q, r.q_norm, dq);
  reinterpret_cast<float4*>(dL_drotations)[i] = dq;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ggd_gaussian_normals(ggd_ctx* ctx, void* stream, int32_t P, const float* rotations, const float* scales,
                                    const float* means3D, const float* viewmatrix, int32_t raw, float* normals) {
  if (!ctx) return GGD_E_INVALID;
  if (P < 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_gaussian_normals: negative P");
  if (!rotations || !scales || !means3D || !viewmatrix || !normals)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_gaussian_normals: NULL pointer");
  if (!aligned16(rotations)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_gaussian_normals: rotations must be 16-byte aligned");
  if (P == 0) return GGD_OK;
  hipLaunchKernelGGL(gaussian_normals_kernel, dim3((P + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), P,
                     rotations, scales, means3D, viewmatrix, raw, normals);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_gaussian_normals_backward(ggd_ctx* ctx, void* stream, int32_t P, const float* rotations,
                                             const float* scales, const float* means3D, const float* viewmatrix, int32_t raw,
                                             const float* dL_dnormals, float* dL_drotations) {
  if (!ctx) return GGD_E_INVALID;
  if (P < 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_gaussian_normals_backward: negative P");
  if (!rotations || !scales || !means3D || !viewmatrix || !dL_dnormals || !dL_drotations)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_gaussian_normals_backward: NULL pointer");
  if (!aligned16(rotations) || !aligned16(dL_drotations))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_gaussian_normals_backward: rotations and dL_drotations must be 16-byte aligned");
  if (P == 0) return GGD_OK;
  hipLaunchKernelGGL(gaussian_normals_backward_kernel, dim3((P + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     P, rotations, scales, means3D, viewmatrix, raw, dL_dnormals, dL_drotations);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
