// ggd_densify.hip -- adaptive density control of a fitted scene: the per-iteration statistics update
// and the clone / split / prune of gaussian_splatting/scene/gaussian_model.py:453-546 as streaming passes.
//
//   statistics   one launch, in place, no host wait: accum += |grad.xy|, denom += 1, max_radii2D = max(.., radii) on visible rows
//   plan         classify every row + reduce (launch 1), scan the block sums (launch 2), write the source map (launch 3), then
//                the ONE read-back of the three segment sizes -- the caller needs the new row count to allocate
//   emit         one gather launch indexed by OUTPUT ELEMENT over the six parameter groups and their Adam moments
//
// The reference runs clone (cat), split (cat), prune, prune in sequence; the final state is a function of each original row
// alone, so it is produced directly (row i of P0, s = exp(scaling), smax = max s, g = accum / denom with 0/0 = 0):
//   hot = g >= max_grad    C = hot && smax <= thr    S = hot && smax > thr    low = sigmoid(opacity) < min_opacity
//   big(x) = world_size test on && x > world_size    prune_self = low || big(smax)    prune_child = low || big(exp(log(smax / 1.6)))
// output segments, each in source order:  0 originals with !S && !prune_self | 1 clones of C && !prune_self (raw copies) |
//   2 first children of S && !prune_child | 3 second children of the same rows.
// (The reference's screen-size test reads max_radii2D after densification_postfix has zeroed it: it never fires, and is not
// restated; max_screen_size only switches the world-size test on.)
// No workgroup waits on another one anywhere in this file: every dependency is a kernel boundary.
#include "ggd_common.h"
#include "ggd_groups.h"
#include "ggd_lanes.h"

namespace {

#include "ggd_scan.inc"

constexpr uint32_t DF_KEEP = 1u, DF_CLONE = 2u, DF_CHILD = 4u;   // per-row flag byte
constexpr int DF_KIND_SHIFT = 30;                                // source map word: segment kind << 30 | parent row
constexpr uint32_t DF_ROW_MASK = (1u << DF_KIND_SHIFT) - 1u;
constexpr float DF_SPLIT_DIV = 1.6f;                             // 0.8 * N, N = 2 children

struct df_layout { size_t flags, sums, counts, src, total; int nb; };

df_layout densify_layout(int32_t P) {
  df_layout t;
  t.nb = (int)(((int64_t)P + SCAN_TILE - 1) / SCAN_TILE);
  t.flags = 0;                                                      // uint8 [nb * SCAN_TILE] (the map step loads 8 at a time)
  t.sums = t.flags + ggd_align((size_t)t.nb * SCAN_TILE);           // uint32 [3][nb]
  t.counts = t.sums + ggd_align((size_t)3 * t.nb * sizeof(uint32_t));   // uint32 [4]: kept, clones, split parents kept, new P
  t.src = t.counts + 256;                                           // uint32 [<= 2 P]: a row yields at most two output rows
  t.total = t.src + ggd_align((size_t)2 * P * sizeof(uint32_t));
  return t;
}

struct df_rule {
  float max_grad, split_thr, min_opacity, world_size;
  int use_world_size;
};

// ------------------------------------------------------------------------------------------------ statistics --
__global__ void __launch_bounds__(256) densify_stats_kernel(const float* __restrict__ grad, const int32_t* __restrict__ radii,
                                                            const uint8_t* __restrict__ filter, float* __restrict__ accum,
                                                            float* __restrict__ denom, float* __restrict__ max_radii, int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int r = radii ? radii[i] : 0;
  const bool visible = filter ? filter[i] != 0 : r > 0;
  if (!visible) return;
  const float gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1];
  accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.0f;
  if (max_radii && radii) max_radii[i] = fmaxf(max_radii[i], (float)r);
}

// ------------------------------------------------------------------------------------------------------ plan --
__device__ __forceinline__ uint32_t densify_row_flags(int i, const float* __restrict__ accum, const float* __restrict__ denom,
                                                      const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                      const df_rule& r) {
  float g = accum[i] / denom[i];
  if (g != g) g = 0.0f;                                  // 0 / 0: a row no frame has seen
  const float* sc = scaling + 3 * (size_t)i;
  const float smax = fmaxf(fmaxf(expf(sc[0]), expf(sc[1])), expf(sc[2]));
  const bool hot = g >= r.max_grad;
  const bool split = hot && smax > r.split_thr;
  const bool clone = hot && smax <= r.split_thr;
  const bool low = 1.0f / (1.0f + expf(-opacity[i])) < r.min_opacity;
  const float child_smax = expf(logf(smax / DF_SPLIT_DIV));   // what get_scaling returns for the child (monotone in s: max commutes)
  const bool prune_self = low || (r.use_world_size && smax > r.world_size);
  const bool prune_child = low || (r.use_world_size && child_smax > r.world_size);
  return (!split && !prune_self ? DF_KEEP : 0u) | (clone && !prune_self ? DF_CLONE : 0u) | (split && !prune_child ? DF_CHILD : 0u);
}

// Launch 1: flags of 2048 rows per workgroup (row = tile base + round * 256 + thread: coalesced; a sum needs no order) and
// their three counts.  PRUNE: the only flag is KEEP = !mask.
template <bool PRUNE>
__global__ void __launch_bounds__(SCAN_THREADS) densify_classify_kernel(int P, const float* __restrict__ accum,
                                                                        const float* __restrict__ denom,
                                                                        const float* __restrict__ scaling,
                                                                        const float* __restrict__ opacity,
                                                                        const uint8_t* __restrict__ mask, df_rule rule,
                                                                        uint8_t* __restrict__ flags, uint32_t* __restrict__ sums,
                                                                        int nb) {
  __shared__ uint32_t lds4[4];
  uint32_t c[3] = {0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int64_t i = (int64_t)blockIdx.x * SCAN_TILE + k * SCAN_THREADS + threadIdx.x;
    uint32_t f = 0u;
    if (i < P) {
      if constexpr (PRUNE) f = mask[i] ? 0u : DF_KEEP;
      else f = densify_row_flags((int)i, accum, denom, scaling, opacity, rule);
    }
    flags[i] = (uint8_t)f;                               // the buffer is whole tiles: the tail past P reads as "nothing"
    c[0] += f & 1u; c[1] += (f >> 1) & 1u; c[2] += (f >> 2) & 1u;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t tot;
    block_exclusive_scan_256(c[j], &tot, lds4);
    if (threadIdx.x == 0) sums[(size_t)j * nb + blockIdx.x] = tot;
  }
}

// Launch 2 (one workgroup): block sums -> exclusive block prefixes, the three totals and the new row count.
__global__ void __launch_bounds__(SCAN_THREADS) densify_blocksums_kernel(uint32_t* __restrict__ sums, int nb,
                                                                         uint32_t* __restrict__ counts) {
  __shared__ uint32_t lds4[4];
  for (int j = 0; j < 3; ++j) scan_blocksums_block(sums + (size_t)j * nb, nb, counts + j, nullptr, lds4);
  __syncthreads();
  if (threadIdx.x == 0) counts[3] = counts[0] + counts[1] + 2u * counts[2];   // (thread 0 wrote all three itself)
}

// Launch 3: source map.  Thread t of workgroup b owns rows b * 2048 + 8 t .. + 7, so every segment keeps source order.
__global__ void __launch_bounds__(SCAN_THREADS) densify_map_kernel(const uint8_t* __restrict__ flags,
                                                                   const uint32_t* __restrict__ prefix, int nb,
                                                                   const uint32_t* __restrict__ counts,
                                                                   uint32_t* __restrict__ src) {
  __shared__ uint32_t lds4[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  const uint2 w = *reinterpret_cast<const uint2*>(flags + base);
  uint32_t f[SCAN_ITEMS];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) f[k] = ((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 0xFFu;
  const uint32_t n_keep = counts[0], n_clone = counts[1], n_child = counts[2];
  const uint32_t seg_base[3] = {0u, n_keep, n_keep + n_clone};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) c += (f[k] >> j) & 1u;
    uint32_t tot;
    uint32_t pos = seg_base[j] + prefix[(size_t)j * nb + blockIdx.x] + block_exclusive_scan_256(c, &tot, lds4);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      if (!((f[k] >> j) & 1u)) continue;
      const uint32_t row = (uint32_t)(base + k);
      if (j < 2) {
        src[pos] = ((uint32_t)j << DF_KIND_SHIFT) | row;
      } else {
        src[pos] = (2u << DF_KIND_SHIFT) | row;
        src[pos + n_child] = (3u << DF_KIND_SHIFT) | row;
      }
      ++pos;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ emit --
struct df_emit_args {
  ggd_row_group g[GG_GROUPS];
  const uint32_t* src;
  const uint32_t* counts;
  const float* noise;        // [2][P0][3]
  uint32_t P0, newP;
};

// xyz of a child: R(q / |q|) (s * noise) + xyz, component c, in the operation order of build_rotation
__device__ __forceinline__ float densify_child_xyz(const df_emit_args& a, uint32_t parent, uint32_t child, uint32_t c) {
  const float* q = a.g[GG_ROTATION].in[0] + 4 * (size_t)parent;
  const float* sc = a.g[GG_SCALING].in[0] + 3 * (size_t)parent;
  const float* nz = a.noise + 3 * ((size_t)child * a.P0 + parent);
  const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
  const float v0 = expf(sc[0]) * nz[0], v1 = expf(sc[1]) * nz[1], v2 = expf(sc[2]) * nz[2];
  float r0, r1, r2;
  if (c == 0) { r0 = 1.0f - 2.0f * (y * y + z * z); r1 = 2.0f * (x * y - r * z); r2 = 2.0f * (x * z + r * y); }
  else if (c == 1) { r0 = 2.0f * (x * y + r * z); r1 = 1.0f - 2.0f * (x * x + z * z); r2 = 2.0f * (y * z - r * x); }
  else { r0 = 2.0f * (x * z - r * y); r1 = 2.0f * (y * z + r * x); r2 = 1.0f - 2.0f * (x * x + y * y); }
  return ((r0 * v0 + r1 * v1) + r2 * v2) + a.g[GG_XYZ].in[0][3 * (size_t)parent + c];
}

// One thread per output float of one group (its parameter and both moments; the walk: ggd_groups.h).  The stores are
// contiguous, the loads follow the source map, which is monotone inside a segment.
__global__ void __launch_bounds__(256) densify_emit_kernel(df_emit_args a) {
  const auto [G, row, col] = ggd_group_walk(a.g);
  const ggd_row_group& grp = a.g[G];
  const uint32_t w = grp.width;
  if (row >= min(a.newP, a.counts[3])) return;
  const uint32_t s = a.src[row];
  const uint32_t kind = s >> DF_KIND_SHIFT, parent = s & DF_ROW_MASK;
  if (parent >= a.P0 || (kind >= 2u && !a.noise)) return;   // (a map of ggd_prune_plan has no children and needs no noise)
  const size_t o = (size_t)row * w + col, i = (size_t)parent * w + col;
  float v;
  if (kind >= 2u && G == GG_XYZ) v = densify_child_xyz(a, parent, kind - 2u, col);
  else if (kind >= 2u && G == GG_SCALING) v = logf(expf(grp.in[0][i]) / DF_SPLIT_DIV);
  else v = grp.in[0][i];
  grp.out[0][o] = v;
  if (grp.out[1]) {
    grp.out[1][o] = kind == 0u ? grp.in[1][i] : 0.0f;
    grp.out[2][o] = kind == 0u ? grp.in[2][i] : 0.0f;
  }
}

// rows of a [P][width] array through the source map (copies only: the statistics arrays of prune_points)
__global__ void __launch_bounds__(256) densify_gather_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             const uint32_t* __restrict__ src, const uint32_t* __restrict__ counts,
                                                             uint32_t P0, uint32_t newP, uint32_t w) {
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t row = (uint32_t)(e / w), col = (uint32_t)(e - (uint64_t)row * w);
  if (row >= min(newP, counts[3])) return;
  const uint32_t parent = src[row] & DF_ROW_MASK;
  if (parent >= P0) return;
  out[e] = in[(size_t)parent * w + col];
}

// classify + scan + map on `s`, then the read-back of {kept, clones, split parents kept, new P}
template <bool PRUNE>
int densify_plan(ggd_ctx* ctx, hipStream_t s, int32_t P, const float* accum, const float* denom, const float* scaling,
                 const float* opacity, const uint8_t* mask, const df_rule& rule, void* tmp, int64_t* counts4) {
  for (int k = 0; k < 4; ++k) counts4[k] = 0;
  const df_layout t = densify_layout(P);
  char* p = static_cast<char*>(tmp);
  uint32_t* counts = reinterpret_cast<uint32_t*>(p + t.counts);
  if (P == 0) {
    GGD_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), s));
    return GGD_OK;
  }
  uint8_t* flags = reinterpret_cast<uint8_t*>(p + t.flags);
  uint32_t* sums = reinterpret_cast<uint32_t*>(p + t.sums);
  uint32_t* src = reinterpret_cast<uint32_t*>(p + t.src);
  hipLaunchKernelGGL(densify_classify_kernel<PRUNE>, dim3(t.nb), dim3(SCAN_THREADS), 0, s, P, accum, denom, scaling, opacity,
                     mask, rule, flags, sums, t.nb);
  hipLaunchKernelGGL(densify_blocksums_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, sums, t.nb, counts);
  hipLaunchKernelGGL(densify_map_kernel, dim3(t.nb), dim3(SCAN_THREADS), 0, s, flags, sums, t.nb, counts, src);
  GGD_HIP(hipGetLastError());
  uint32_t h[4] = {0, 0, 0, 0};
  GGD_HIP(hipMemcpyAsync(h, counts, sizeof(h), hipMemcpyDeviceToHost, s));
  GGD_HIP(hipStreamSynchronize(s));                      // the one host wait of a densification
  for (int k = 0; k < 4; ++k) counts4[k] = (int64_t)h[k];
  return GGD_OK;
}

}  // namespace

extern "C" size_t ggd_densify_tmp_bytes(int32_t P) { return (P < 0 || P > GG_MAX_POINTS) ? 0 : densify_layout(P).total; }

extern "C" int ggd_densify_stats(ggd_ctx* ctx, void* stream, int32_t P, const float* grad_means2D, const int32_t* radii,
                                 const uint8_t* filter, float* accum, float* denom, float* max_radii2D) {
  if (!ctx) return GGD_E_INVALID;
  if (P < 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_stats: negative P");
  if (!radii && !filter) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_stats: radii or filter must be given");
  if (max_radii2D && !radii) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_stats: max_radii2D needs radii");
  if (P == 0) return GGD_OK;
  if (!grad_means2D || !accum || !denom) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_stats: NULL pointer");
  hipLaunchKernelGGL(densify_stats_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     grad_means2D, radii, filter, accum, denom, max_radii2D, P);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_densify_plan(ggd_ctx* ctx, void* stream, int32_t P, const float* accum, const float* denom,
                                const float* scaling, const float* opacity, float max_grad, float split_threshold,
                                float min_opacity, int32_t use_world_size, float world_size, void* tmp, size_t tmp_bytes,
                                int64_t* counts4) {
  if (!ctx) return GGD_E_INVALID;
  if (!counts4) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_plan: NULL counts");
  if (int rc = ggd_check_tmp(ctx, "ggd_densify_plan", P, tmp, tmp_bytes, densify_layout(P).total)) return rc;
  if (!(max_grad > 0.0f)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_plan: max_grad must be > 0 (a clone's zero statistic would split)");
  if (P > 0 && (!accum || !denom || !scaling || !opacity)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_plan: NULL pointer");
  const df_rule rule = {max_grad, split_threshold, min_opacity, world_size, use_world_size != 0};
  return densify_plan<false>(ctx, static_cast<hipStream_t>(stream), P, accum, denom, scaling, opacity, nullptr, rule, tmp, counts4);
}

extern "C" int ggd_prune_plan(ggd_ctx* ctx, void* stream, int32_t P, const uint8_t* mask, void* tmp, size_t tmp_bytes,
                              int64_t* counts4) {
  if (!ctx) return GGD_E_INVALID;
  if (!counts4) return ggd_fail(ctx, GGD_E_INVALID, "ggd_prune_plan: NULL counts");
  if (int rc = ggd_check_tmp(ctx, "ggd_prune_plan", P, tmp, tmp_bytes, densify_layout(P).total)) return rc;
  if (P > 0 && !mask) return ggd_fail(ctx, GGD_E_INVALID, "ggd_prune_plan: NULL mask");
  return densify_plan<true>(ctx, static_cast<hipStream_t>(stream), P, nullptr, nullptr, nullptr, nullptr, mask, df_rule(), tmp, counts4);
}

extern "C" int ggd_densify_emit(ggd_ctx* ctx, void* stream, int32_t P, int32_t new_P, int32_t M, const float* const* in18,
                                float* const* out18, const float* noise, const void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (int rc = ggd_check_tmp(ctx, "ggd_densify_emit", P, tmp, tmp_bytes, densify_layout(P).total)) return rc;
  if (new_P < 0 || (int64_t)new_P > 2 * (int64_t)P) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_emit: new_P must be in [0, 2 P]");
  if (int rc = ggd_groups_check_M(ctx, "ggd_densify_emit", M)) return rc;
  if (new_P == 0) return GGD_OK;
  const df_layout t = densify_layout(P);
  const char* p = static_cast<const char*>(tmp);
  df_emit_args a;
  a.src = reinterpret_cast<const uint32_t*>(p + t.src);
  a.counts = reinterpret_cast<const uint32_t*>(p + t.counts);
  a.noise = noise;
  a.P0 = (uint32_t)P;
  a.newP = (uint32_t)new_P;
  uint64_t blocks;
  if (int rc = ggd_groups_fill(ctx, "ggd_densify_emit", M, new_P, in18, out18, a.g, blocks)) return rc;
  hipLaunchKernelGGL(densify_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_densify_gather(ggd_ctx* ctx, void* stream, int32_t P, int32_t new_P, int32_t width, const float* in,
                                  float* out, const void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (int rc = ggd_check_tmp(ctx, "ggd_densify_gather", P, tmp, tmp_bytes, densify_layout(P).total)) return rc;
  if (new_P < 0 || (int64_t)new_P > 2 * (int64_t)P) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_gather: new_P must be in [0, 2 P]");
  if (width < 1 || width > 64) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_gather: width must be in [1, 64]");
  if (new_P == 0) return GGD_OK;
  if (!in || !out) return ggd_fail(ctx, GGD_E_INVALID, "ggd_densify_gather: NULL pointer");
  const df_layout t = densify_layout(P);
  const char* p = static_cast<const char*>(tmp);
  const uint64_t blocks = ((uint64_t)new_P * (uint32_t)width + 255u) / 256u;
  hipLaunchKernelGGL(densify_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), in, out,
                     reinterpret_cast<const uint32_t*>(p + t.src), reinterpret_cast<const uint32_t*>(p + t.counts), (uint32_t)P,
                     (uint32_t)new_P, (uint32_t)width);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
