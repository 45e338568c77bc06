// ggd_adam.hip -- the fitting loop's optimizer step: sparse Adam over up to eight [N][width] float32
// parameter groups in ONE launch, in place.  Only the rows the frame saw (visible[i] != 0, or radii[i] > 0) are read and
// written; every other row keeps its parameter and both moments, and none of its bytes is loaded.
//
// Per element of a visible row, fp32, every operation rounded on its own (the library is built with -ffp-contract=off and
// correctly rounded division / square root, so the order below defines the bits):
//   m' = (b1 * m) + ((1 - b1) * g)      v' = (b2 * v) + (((1 - b2) * g) * g)      p' = p + (((-lr) * m') / (sqrt(v') + eps))
// No bias correction, no step counter: the published adamUpdate rule of the accelerated 3DGS rasterizer.
//
// Shape: a streaming pass.  A group is its N * width floats in memory order, cut into a scalar head (up to the first 16-byte
// boundary), 16-byte chunks, and a scalar tail; one thread owns one chunk (or one head / tail element) of the parameter, the
// gradient and both moments.  The chunk form needs the four base pointers congruent modulo 16; a group whose pointers are
// not is run element by element.  The row of an element is element / width by a multiply with a per-group constant computed
// on the host.  A chunk whose elements are all visible moves as four 16-byte loads and three 16-byte stores; a chunk with
// none returns after the visibility bytes; a chunk that straddles a visible and an invisible row falls back to its visible
// elements one by one, so the promise above holds per row and not per chunk.  Every group owns a range of workgroups computed
// on the host; the table travels by value in the kernel arguments.  No workgroup waits on another.
#include "ggd_common.h"
#include "ggd_groups.h"

namespace {

constexpr int AD_MAX_GROUPS = 8;
constexpr int AD_THREADS = 256;

struct ad_group {
  float* param; const float* grad; float* m; float* v;
  uint32_t len;          // N * width floats
  uint32_t width;
  uint32_t head;         // scalar elements in front of the first chunk (0..3)
  uint32_t n_chunks;     // 16-byte chunks (0: the whole group is run element by element)
  uint32_t first_block;  // this group's first workgroup of the launch (0xFFFFFFFF: no workgroups)
  uint32_t div_mul;      // element / width = (element * div_mul) >> div_shift for element < 2^31
  uint32_t div_shift;
  float lr, eps;
};
struct ad_args {
  ad_group g[AD_MAX_GROUPS];
  const uint8_t* visible;
  const int32_t* radii;
  float b1, b2;
};

// Division of a dividend below 2^31 by the constant d >= 1 (Granlund & Montgomery, N = 31): with l = ceil(log2 d) and
// mul = floor(2^(31 + l) / d) + 1 one has 2^(31 + l) < mul * d <= 2^(31 + l) + 2^l, which makes (n * mul) >> (31 + l) the
// exact quotient; mul < 2^32 and n * mul < 2^63.
void ad_divider(uint32_t d, uint32_t* mul, uint32_t* shift) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  *mul = (uint32_t)((1ull << (31 + l)) / d + 1ull);
  *shift = 31 + l;
}

__device__ __forceinline__ uint32_t ad_row(uint32_t e, const ad_group& g) {
  return (uint32_t)(((uint64_t)e * g.div_mul) >> g.div_shift);
}

__device__ __forceinline__ bool ad_visible(const ad_args& a, uint32_t row) {
  return a.visible ? a.visible[row] != 0 : a.radii[row] > 0;
}

__device__ __forceinline__ void ad_update(float& p, float g, float& m, float& v, float b1, float b2, float c1, float c2, float nlr,
                                          float eps) {
  m = (b1 * m) + (c1 * g);
  v = (b2 * v) + ((c2 * g) * g);
  p = p + ((nlr * m) / (sqrtf(v) + eps));
}

__device__ __forceinline__ void ad_one(const ad_group& g, uint32_t e, float b1, float b2, float c1, float c2) {
  float p = g.param[e], m = g.m[e], v = g.v[e];
  ad_update(p, g.grad[e], m, v, b1, b2, c1, c2, -g.lr, g.eps);
  g.param[e] = p; g.m[e] = m; g.v[e] = v;
}

__global__ void __launch_bounds__(AD_THREADS) adam_sparse_kernel(ad_args a) {
  const ad_group& g = a.g[ggd_block_group(a.g)];
  const uint32_t t = (blockIdx.x - g.first_block) * AD_THREADS + threadIdx.x;
  const float b1 = a.b1, b2 = a.b2, c1 = 1.0f - a.b1, c2 = 1.0f - a.b2;
  if (t >= g.n_chunks) {                                 // head, then tail, one element per thread
    const uint32_t s = t - g.n_chunks;
    const uint32_t e = s < g.head ? s : 4u * g.n_chunks + s;
    if (e >= g.len) return;
    if (ad_visible(a, ad_row(e, g))) ad_one(g, e, b1, b2, c1, c2);
    return;
  }
  const uint32_t e0 = g.head + 4u * t;
  const uint32_t r0 = ad_row(e0, g), r3 = ad_row(e0 + 3u, g);
  const bool v0 = ad_visible(a, r0);
  bool vis[4] = {v0, v0, v0, v0};
  if (r3 != r0) {                                        // the chunk crosses a row edge (width 1: three of them)
    const uint32_t r1 = ad_row(e0 + 1u, g), r2 = ad_row(e0 + 2u, g);
    vis[3] = ad_visible(a, r3);
    vis[1] = r1 == r0 ? v0 : r1 == r3 ? vis[3] : ad_visible(a, r1);
    vis[2] = r2 == r0 ? v0 : r2 == r3 ? vis[3] : ad_visible(a, r2);
  }
  const int n_vis = (int)vis[0] + (int)vis[1] + (int)vis[2] + (int)vis[3];
  if (n_vis == 0) return;
  if (n_vis < 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (vis[k]) ad_one(g, e0 + k, b1, b2, c1, c2);
    return;
  }
  float4 p = *reinterpret_cast<const float4*>(g.param + e0);
  const float4 gr = *reinterpret_cast<const float4*>(g.grad + e0);
  float4 m = *reinterpret_cast<const float4*>(g.m + e0);
  float4 v = *reinterpret_cast<const float4*>(g.v + e0);
  const float nlr = -g.lr, eps = g.eps;
  ad_update(p.x, gr.x, m.x, v.x, b1, b2, c1, c2, nlr, eps);
  ad_update(p.y, gr.y, m.y, v.y, b1, b2, c1, c2, nlr, eps);
  ad_update(p.z, gr.z, m.z, v.z, b1, b2, c1, c2, nlr, eps);
  ad_update(p.w, gr.w, m.w, v.w, b1, b2, c1, c2, nlr, eps);
  *reinterpret_cast<float4*>(g.param + e0) = p;
  *reinterpret_cast<float4*>(g.m + e0) = m;
  *reinterpret_cast<float4*>(g.v + e0) = v;
}

}  // namespace

extern "C" int ggd_adam_sparse(ggd_ctx* ctx, void* stream, int32_t N, int32_t n_groups, const ggd_adam_group* groups,
                               const uint8_t* visible, const int32_t* radii, float beta1, float beta2) {
  if (!ctx) return GGD_E_INVALID;
  if (N < 0 || N > GG_MAX_POINTS) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: N must be in [0, 2^26]");
  if (n_groups < 1 || n_groups > AD_MAX_GROUPS) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: n_groups must be in [1, 8]");
  if (!groups) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: NULL group table");
  if ((visible != nullptr) == (radii != nullptr))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: exactly one of visible and radii must be given");
  ad_args a;
  a.visible = visible; a.radii = radii; a.b1 = beta1; a.b2 = beta2;
  uint64_t blocks = 0;
  for (int k = 0; k < AD_MAX_GROUPS; ++k) {
    ad_group& d = a.g[k];
    d = ad_group();
    d.first_block = 0xFFFFFFFFu;
    if (k >= n_groups) continue;
    const ggd_adam_group& s = groups[k];
    if (s.width < 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: negative width");
    if ((int64_t)N * s.width >= (1ll << 31)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: N * width must be below 2^31");
    if (!s.grad || s.width == 0) continue;               // skipped group
    if (!s.param || !s.exp_avg || !s.exp_avg_sq) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: NULL parameter or moment pointer");
    const uintptr_t at[4] = {reinterpret_cast<uintptr_t>(s.param), reinterpret_cast<uintptr_t>(s.grad),
                             reinterpret_cast<uintptr_t>(s.exp_avg), reinterpret_cast<uintptr_t>(s.exp_avg_sq)};
    if ((at[0] | at[1] | at[2] | at[3]) & 3u) return ggd_fail(ctx, GGD_E_INVALID, "ggd_adam_sparse: a pointer is not 4-byte aligned");
    d.param = s.param; d.grad = s.grad; d.m = s.exp_avg; d.v = s.exp_avg_sq;
    d.width = (uint32_t)s.width;
    d.len = (uint32_t)((int64_t)N * s.width);
    d.lr = s.lr; d.eps = s.eps;
    ad_divider(d.width, &d.div_mul, &d.div_shift);
    const bool congruent = (at[0] & 15u) == (at[1] & 15u) && (at[0] & 15u) == (at[2] & 15u) && (at[0] & 15u) == (at[3] & 15u);
    if (congruent) {
      d.head = (uint32_t)(((16u - (at[0] & 15u)) & 15u) / 4u);
      if (d.head > d.len) d.head = d.len;
      d.n_chunks = (d.len - d.head) / 4u;
    }
    if (d.len == 0) continue;
    d.first_block = (uint32_t)blocks;
    // threads: the chunks, then the head and the tail (len - 4 n_chunks elements together)
    blocks += ((uint64_t)d.n_chunks + (d.len - 4u * d.n_chunks) + AD_THREADS - 1) / AD_THREADS;
  }
  if (blocks == 0) return GGD_OK;                         // N == 0, or every group skipped
  // a group without workgroups must not catch the group search: it keeps 0xFFFFFFFF, above every block index
  hipLaunchKernelGGL(adam_sparse_kernel, dim3((unsigned)blocks), dim3(AD_THREADS), 0, static_cast<hipStream_t>(stream), a);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
