// ggd_mcmc.hip -- density control of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024) under a fixed
// row budget: the relocation values (its compute_relocation op), relocate_gs, add_new_gs and the
// per-iteration position noise, restated from the published source as streaming passes.
//
//   weights   launch 1: per row w = alive ? max(1, round(sigmoid(x) * 2^20)) : 0 (uint32), its exclusive prefix inside the row's
//             2048-row tile, the tile's sum, count = 0
//   tiles     launch 2 (one workgroup): tile sums -> 64-bit exclusive tile prefixes and the grand total W
//   sample    launch 3: destination j with draw d picks tau = floor(d * W / 2^32) (exact: the high word of (d << 32) * W) and the
//             source is the row whose interval [C_i, C_i + w_i) holds tau -- two binary searches, over the tile prefixes and
//             inside the tile; count[source] += 1 (an integer atomic: the sum does not depend on the order)
//   values    launch 4 (pass A): every row with count > 0 gets its new raw opacity and raw scales in scratch, N = min(51, 1 + count)
//   emit      launch 5 (pass B): relocate, in place: a destination copies its source's xyz, f_dc, f_rest and rotation and takes
//             the source's scratch values; a sampled source takes its own and its Adam moments become 0.  add, out of place: old
//             rows are copied (sampled sources as above), row P + k is a copy of source s_k with zero moments.
// The choice of sources is a pure function of the integer weights and the draws: no float prefix sum exists anywhere, so it is
// the same from run to run and on every machine.  Hazards of the in-place pass B: a source is an alive row and a destination a
// dead one, so no row is both; a destination reads only columns of its source that pass B never writes (xyz, f_dc, f_rest,
// rotation) and the scratch of pass A; the old opacity and scales of a source are read by pass A alone, a kernel boundary before
// their overwrite.  No workgroup waits on another one anywhere in this file: every dependency is a kernel boundary.
//
// Per-row rule of the values (x the raw opacity, N the ratio):  sp = softplus(x) = -log(1 - o),  o = -expm1(-sp),
//   o' = -expm1(-sp / N) = 1 - (1 - o)^(1/N)      D = sum_{i=1..N} sum_{k<i} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1)
//   new raw scale = raw scale + log(o / D)        new raw opacity = log(expm1(sp / N)), o' clamped to [0.005, 1 - 2^-23]
// 1 - o is never formed by subtraction.  The inner sums over i collapse (sum_{i=k+1..N} C(i-1, k) = C(N, k+1)), so D is N terms
// of alternating sign; their cancellation reaches four digits at N = 51, and the pass (which runs on the sampled rows only, once
// per relocation) evaluates the whole rule in fp64.
#include "ggd_common.h"
#include "ggd_groups.h"
#include "ggd_lanes.h"
#include "ggd_math.h"

namespace {

using namespace ggdm;

#include "ggd_scan.inc"

constexpr int MC_NMAX = 51;
constexpr uint32_t MC_NONE = 0xFFFFFFFFu;                // sources[]: "this row is no destination"
constexpr float MC_WEIGHT_ONE = 1048576.0f;              // 2^20: a 2048-row tile's sum fits 32 bits
constexpr float MC_DEAD_OPACITY = 0.005f;
// smallest float >= logit(0.005) and largest float <= logit(1 - 2^-23): sigmoid of the clamped raw opacity stays inside the bounds
constexpr float MC_RAW_LO = -0x1.52c58p+2f, MC_RAW_HI = 0x1.fe2804p+3f;

// C(n, k) for n <= 51, exact in fp64 (C(51, 25) < 2^48), built once at compile time
struct mc_binom_table {
  double v[MC_NMAX + 1][MC_NMAX + 1];
  constexpr mc_binom_table() : v() {
    for (int n = 0; n <= MC_NMAX; ++n)
      for (int k = 0; k <= MC_NMAX; ++k) v[n][k] = k == 0 ? 1.0 : (n == 0 || k > n) ? 0.0 : v[n - 1][k - 1] + v[n - 1][k];
  }
};
__device__ const mc_binom_table MC_BINOM = mc_binom_table();

struct mc_layout { size_t w, cw, tile, counts, sources, newv, total; int nb; };

mc_layout mcmc_layout(int32_t P, int32_t n_dest) {
  mc_layout t;
  t.nb = (int)(((int64_t)P + SCAN_TILE - 1) / SCAN_TILE);
  t.w = 0;                                                                   // uint32 [nb * SCAN_TILE]
  t.cw = t.w + ggd_align((size_t)t.nb * SCAN_TILE * sizeof(uint32_t));       // uint32 [nb * SCAN_TILE]: exclusive prefix in the tile
  t.tile = t.cw + ggd_align((size_t)t.nb * SCAN_TILE * sizeof(uint32_t));    // uint64 [nb + 1]: tile prefixes, then W
  t.counts = t.tile + ggd_align(((size_t)t.nb + 1) * sizeof(uint64_t));      // uint32 [P]
  t.sources = t.counts + ggd_align((size_t)P * sizeof(uint32_t));            // uint32 [n_dest]
  t.newv = t.sources + ggd_align((size_t)n_dest * sizeof(uint32_t));         // float [P][4]: raw opacity, raw scales
  t.total = t.newv + ggd_align((size_t)P * 4 * sizeof(float));
  return t;
}

// ----------------------------------------------------------------------------------------------------- values --
// D(o', N) as N terms (see the head of the file)
__device__ __forceinline__ double mcmc_denominator(double op, int N) {
  double sum = 0.0, p = op;
  for (int k = 0; k < N; ++k) {
    const double term = MC_BINOM.v[N][k + 1] * p / sqrt((double)(k + 1));
    sum += (k & 1) ? -term : term;
    p *= op;
  }
  return sum;
}

__device__ __forceinline__ double mcmc_softplus(double x) { return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)); }

// new raw opacity and log(o / D) of a row with raw opacity x that was sampled N - 1 times
__device__ __forceinline__ void mcmc_row_values(float x, int N, float& raw_opacity, double& log_scale_factor) {
  const double sp = mcmc_softplus((double)x), t = sp / (double)N;
  const double o = -expm1(-sp), op = -expm1(-t);
  const float raw = (float)log(expm1(t));
  raw_opacity = fminf(fmaxf(raw, MC_RAW_LO), MC_RAW_HI);
  log_scale_factor = log(o / mcmc_denominator(op, N));
}

// ---------------------------------------------------------------------------------------------------- weights --
// Thread t of workgroup b owns rows b * 2048 + 8 t .. + 7.  mask: uint8 [P] (set = dead) or NULL; without a mask a row is dead when
// RULE and sigmoid(x) <= 0.005 (RULE false: every row is alive, add_new_gs).
template <bool RULE>
__global__ void __launch_bounds__(SCAN_THREADS) mcmc_weights_kernel(int P, const float* __restrict__ opacity,
                                                                    const uint8_t* __restrict__ mask, uint32_t* __restrict__ w,
                                                                    uint32_t* __restrict__ cw, uint64_t* __restrict__ tile,
                                                                    uint32_t* __restrict__ counts) {
  __shared__ uint32_t lds4[4];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int64_t i = base + k;
    v[k] = 0u;
    if (i < P) {
      const float o = act_sigmoid(opacity[i]);
      const bool dead = mask ? mask[i] != 0 : (RULE && o <= MC_DEAD_OPACITY);
      if (!dead) v[k] = max(1u, (uint32_t)rintf(o * MC_WEIGHT_ONE));   // (a NaN opacity converts to 0: weight 1)
      counts[i] = 0u;
    }
    c += v[k];
  }
  uint32_t tot;
  uint32_t run = block_exclusive_scan_256(c, &tot, lds4);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {                 // the two arrays are whole tiles: the tail past P holds weight 0
    w[base + k] = v[k];
    cw[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) tile[blockIdx.x] = tot;
}

// One workgroup: tile sums -> exclusive 64-bit prefixes in place, tile[nb] = W.  Thread t owns a contiguous chunk of the tiles.
__global__ void __launch_bounds__(SCAN_THREADS) mcmc_tiles_kernel(uint64_t* __restrict__ tile, int nb) {
  __shared__ uint64_t part[SCAN_THREADS];
  const int chunk = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
  const int lo = min(nb, (int)threadIdx.x * chunk), hi = min(nb, lo + chunk);
  uint64_t s = 0;
  for (int i = lo; i < hi; ++i) s += tile[i];
  part[threadIdx.x] = s;
  __syncthreads();
  uint64_t run = 0;
  for (int t = 0; t < (int)threadIdx.x; ++t) run += part[t];
  for (int i = lo; i < hi; ++i) {
    const uint64_t v = tile[i];
    tile[i] = run;
    run += v;
  }
  if (threadIdx.x == SCAN_THREADS - 1) tile[nb] = run;
}

// ----------------------------------------------------------------------------------------------------- sample --
// ROWS: destination j is row j, and only the rows of weight 0 are destinations (relocate); otherwise j is the j-th new row (add).
template <bool ROWS>
__global__ void __launch_bounds__(256) mcmc_sample_kernel(int P, int n_dest, const int64_t* __restrict__ draws,
                                                          const uint32_t* __restrict__ w, const uint32_t* __restrict__ cw,
                                                          const uint64_t* __restrict__ tile, int nb,
                                                          uint32_t* __restrict__ counts, uint32_t* __restrict__ sources) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_dest) return;
  const uint64_t W = tile[nb];
  if ((ROWS && w[j] != 0u) || W == 0u) { sources[j] = MC_NONE; return; }
  const uint64_t d = (uint64_t)draws[j] & 0xFFFFFFFFull;
  const uint64_t tau = __umul64hi(d << 32, W);           // floor(d * W / 2^32) < W
  int lo = 0, hi = nb;                                   // the last tile whose prefix is <= tau (tile[0] = 0: there is one)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile[mid] <= tau) lo = mid; else hi = mid;
  }
  const uint32_t r = (uint32_t)(tau - tile[lo]);         // < the tile's sum
  const uint32_t* c = cw + (size_t)lo * SCAN_TILE;
  int a = 0, b = SCAN_TILE;                              // the last row of the tile whose prefix is <= r: its weight is > 0
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (c[mid] <= r) a = mid; else b = mid;
  }
  const uint32_t src = (uint32_t)lo * SCAN_TILE + (uint32_t)a;
  if (src >= (uint32_t)P) { sources[j] = MC_NONE; return; }
  sources[j] = src;
  atomicAdd(counts + src, 1u);
}

__global__ void __launch_bounds__(256) mcmc_values_kernel(int P, const float* __restrict__ opacity,
                                                          const float* __restrict__ scaling, const uint32_t* __restrict__ counts,
                                                          float* __restrict__ newv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const uint32_t cnt = counts[i];
  if (cnt == 0u) return;
  float raw;
  double lf;
  mcmc_row_values(opacity[i], (int)min(cnt, (uint32_t)(MC_NMAX - 1)) + 1, raw, lf);
  float* o = newv + 4 * (size_t)i;
  o[0] = raw;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[1 + c] = (float)((double)scaling[3 * (size_t)i + c] + lf);
}

// ------------------------------------------------------------------------------------------------------- emit --
struct mc_emit_args {
  ggd_row_group g[GG_GROUPS];   // relocate: in and out are the same arrays
  const uint32_t* sources;
  const uint32_t* counts;
  const float* newv;
  uint32_t P, rows;          // rows the launch covers: P (relocate) or P + num (add)
};

// One thread per float of one group's rows (its parameter and both moments; the walk: ggd_groups.h).
template <bool ADD>
__global__ void __launch_bounds__(256) mcmc_emit_kernel(mc_emit_args a) {
  const auto [G, row, col] = ggd_group_walk(a.g);
  const ggd_row_group& grp = a.g[G];
  const uint32_t w = grp.width;
  if (row >= a.rows) return;
  uint32_t src = row;
  bool dest = false;
  if (ADD) {
    if (row >= a.P) { src = a.sources[row - a.P]; dest = true; }
  } else {
    const uint32_t s = a.sources[row];
    if (s != MC_NONE) { src = s; dest = true; }
  }
  if (src >= a.P) return;                                                    // (a plan never holds one)
  const bool sampled = a.counts[src] != 0u;
  if (!ADD && !dest && !sampled) return;                                     // relocate: the row is not touched
  const size_t o = (size_t)row * w + col, i = (size_t)src * w + col;
  const bool fresh = sampled && (G == GG_OPACITY || G == GG_SCALING);
  if (ADD || dest || fresh)
    grp.out[0][o] = fresh ? a.newv[4 * (size_t)src + (G == GG_SCALING ? 1u + col : 0u)] : grp.in[0][i];
  if (!grp.out[1]) return;
  if (ADD) {
    grp.out[1][o] = (dest || sampled) ? 0.0f : grp.in[1][i];
    grp.out[2][o] = (dest || sampled) ? 0.0f : grp.in[2][i];
  } else if (!dest) {                                                        // a sampled source; a destination keeps its moments
    grp.out[1][o] = 0.0f;
    grp.out[2][o] = 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------ noise --
// xyz += Sigma (((xi * gate) * noise_lr) * xyz_lr), Sigma = R S^2 R^T applied as R (S^2 (R^T v)), one thread per row
__global__ void __launch_bounds__(256) mcmc_noise_kernel(int P, float* __restrict__ xyz, const float* __restrict__ scaling,
                                                         const float* __restrict__ rotation, const float* __restrict__ opacity,
                                                         const float* __restrict__ noise, float noise_lr, float xyz_lr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float4 qr = *reinterpret_cast<const float4*>(rotation + 4 * (size_t)i);
  float norm;
  const float4 q = act_normalize(qr, norm);
  float R[3][3];
  quat_rotation(q, R);
  const float one_minus_o = 1.0f / (1.0f + expf(opacity[i]));               // sigmoid(-x)
  const float gate = 1.0f / (1.0f + expf(-100.0f * (one_minus_o - 0.995f)));
  float v[3], u[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = ((noise[3 * (size_t)i + c] * gate) * noise_lr) * xyz_lr;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s = expf(scaling[3 * (size_t)i + c]);
    u[c] = (s * s) * ((R[0][c] * v[0] + R[1][c] * v[1]) + R[2][c] * v[2]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) xyz[3 * (size_t)i + c] += (R[c][0] * u[0] + R[c][1] * u[1]) + R[c][2] * u[2];
}

// ------------------------------------------------------------------------------------------- compute_relocation --
// the op on activated values: o' = 1 - (1 - o)^(1/N) as -expm1(log1p(-o) / N), s' = s o / D; no clamp of o' (the caller's)
__global__ void __launch_bounds__(256) mcmc_relocation_kernel(int n, const float* __restrict__ opacities,
                                                              const float* __restrict__ scales, const int32_t* __restrict__ ratios,
                                                              float* __restrict__ new_opacities, float* __restrict__ new_scales) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int N = min(max(ratios[i], 1), MC_NMAX);
  const double o = (double)opacities[i];
  const double op = -expm1(log1p(-o) / (double)N);
  const double f = o / mcmc_denominator(op, N);
  new_opacities[i] = (float)op;
#pragma unroll
  for (int c = 0; c < 3; ++c) new_scales[3 * (size_t)i + c] = (float)((double)scales[3 * (size_t)i + c] * f);
}

int mcmc_check_tmp(ggd_ctx* ctx, const char* who, int32_t P, int32_t n_dest, const void* tmp, size_t tmp_bytes) {
  const bool P_ok = P >= 0 && P <= GG_MAX_POINTS;        // (a refused P is reported first, by the shared check)
  if (P_ok && (n_dest < 0 || n_dest > GG_MAX_POINTS)) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": the number of destinations must be in [0, 2^26]");
  return ggd_check_tmp(ctx, who, P, tmp, tmp_bytes, mcmc_layout(P, n_dest).total);
}

struct mc_views { uint32_t *w, *cw; uint64_t* tile; uint32_t *counts, *sources; float* newv; int nb; };

mc_views mcmc_views(void* tmp, int32_t P, int32_t n_dest) {
  const mc_layout t = mcmc_layout(P, n_dest);
  char* p = static_cast<char*>(tmp);
  return {reinterpret_cast<uint32_t*>(p + t.w), reinterpret_cast<uint32_t*>(p + t.cw), reinterpret_cast<uint64_t*>(p + t.tile),
          reinterpret_cast<uint32_t*>(p + t.counts), reinterpret_cast<uint32_t*>(p + t.sources),
          reinterpret_cast<float*>(p + t.newv), t.nb};
}

// launches 1 - 4 (P > 0, n_dest > 0)
template <bool ROWS>
void mcmc_plan(hipStream_t s, int32_t P, int32_t n_dest, const float* opacity, const float* scaling, const uint8_t* mask,
               const int64_t* draws, const mc_views& v) {
  hipLaunchKernelGGL(mcmc_weights_kernel<ROWS>, dim3(v.nb), dim3(SCAN_THREADS), 0, s, P, opacity, mask, v.w, v.cw, v.tile, v.counts);
  hipLaunchKernelGGL(mcmc_tiles_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, v.tile, v.nb);
  hipLaunchKernelGGL(mcmc_sample_kernel<ROWS>, dim3((unsigned)((n_dest + 255) / 256)), dim3(256), 0, s, P, n_dest, draws, v.w, v.cw,
                     v.tile, v.nb, v.counts, v.sources);
  hipLaunchKernelGGL(mcmc_values_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, opacity, scaling, v.counts, v.newv);
}

}  // namespace

extern "C" size_t ggd_mcmc_tmp_bytes(int32_t P, int32_t n_dest) {
  return (P < 0 || P > GG_MAX_POINTS || n_dest < 0 || n_dest > GG_MAX_POINTS) ? 0 : mcmc_layout(P, n_dest).total;
}

extern "C" int ggd_mcmc_relocate(ggd_ctx* ctx, void* stream, int32_t P, int32_t M, float* const* io18, const uint8_t* dead_mask,
                                 const int64_t* draws, void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (int rc = mcmc_check_tmp(ctx, "ggd_mcmc_relocate", P, P, tmp, tmp_bytes)) return rc;
  const mc_views v = mcmc_views(tmp, P, P);
  mc_emit_args a = {{}, v.sources, v.counts, v.newv, (uint32_t)P, (uint32_t)P};
  uint64_t blocks;
  if (int rc = ggd_groups_check_M(ctx, "ggd_mcmc_relocate", M)) return rc;
  if (int rc = ggd_groups_fill(ctx, "ggd_mcmc_relocate", M, P, io18, io18, a.g, blocks)) return rc;
  if (P == 0) return GGD_OK;
  if (!draws) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_relocate: NULL draws");
  hipStream_t s = static_cast<hipStream_t>(stream);
  mcmc_plan<true>(s, P, P, a.g[GG_OPACITY].in[0], a.g[GG_SCALING].in[0], dead_mask, draws, v);
  hipLaunchKernelGGL(mcmc_emit_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_mcmc_add_plan(ggd_ctx* ctx, void* stream, int32_t P, int32_t num, const float* opacity, const float* scaling,
                                 const int64_t* draws, void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (int rc = mcmc_check_tmp(ctx, "ggd_mcmc_add_plan", P, num, tmp, tmp_bytes)) return rc;
  if (P == 0 && num > 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_add_plan: no row to sample from");
  if (num == 0) return GGD_OK;
  if (!opacity || !scaling || !draws) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_add_plan: NULL pointer");
  mcmc_plan<false>(static_cast<hipStream_t>(stream), P, num, opacity, scaling, nullptr, draws, mcmc_views(tmp, P, num));
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_mcmc_add_emit(ggd_ctx* ctx, void* stream, int32_t P, int32_t num, int32_t M, const float* const* in18,
                                 float* const* out18, const void* tmp, size_t tmp_bytes) {
  if (!ctx) return GGD_E_INVALID;
  if (int rc = mcmc_check_tmp(ctx, "ggd_mcmc_add_emit", P, num, tmp, tmp_bytes)) return rc;
  if (P == 0 && num > 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_add_emit: no row to sample from");
  if (num == 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_add_emit: num must be > 0 (without new rows there is no plan in tmp)");
  const mc_views v = mcmc_views(const_cast<void*>(tmp), P, num);
  mc_emit_args a = {{}, v.sources, v.counts, v.newv, (uint32_t)P, (uint32_t)(P + num)};
  uint64_t blocks;
  if (int rc = ggd_groups_check_M(ctx, "ggd_mcmc_add_emit", M)) return rc;
  if (int rc = ggd_groups_fill(ctx, "ggd_mcmc_add_emit", M, P + num, in18, out18, a.g, blocks)) return rc;
  hipLaunchKernelGGL(mcmc_emit_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_mcmc_noise(ggd_ctx* ctx, void* stream, int32_t P, float* xyz, const float* scaling, const float* rotation,
                              const float* opacity, const float* noise, float noise_lr, float xyz_lr) {
  if (!ctx) return GGD_E_INVALID;
  if (P < 0 || P > GG_MAX_POINTS) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_noise: P must be in [0, 2^26]");
  if (P == 0) return GGD_OK;
  if (!xyz || !scaling || !rotation || !opacity || !noise) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_noise: NULL pointer");
  if (reinterpret_cast<uintptr_t>(rotation) & 15u) return ggd_fail(ctx, GGD_E_INVALID, "ggd_mcmc_noise: rotation must be 16-byte aligned");
  hipLaunchKernelGGL(mcmc_noise_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), P, xyz,
                     scaling, rotation, opacity, noise, noise_lr, xyz_lr);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

extern "C" int ggd_compute_relocation(ggd_ctx* ctx, void* stream, int32_t n, const float* opacities, const float* scales,
                                      const int32_t* ratios, float* new_opacities, float* new_scales) {
  if (!ctx) return GGD_E_INVALID;
  if (n < 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_compute_relocation: negative n");
  if (n == 0) return GGD_OK;
  if (!opacities || !scales || !ratios || !new_opacities || !new_scales)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_compute_relocation: NULL pointer");
  hipLaunchKernelGGL(mcmc_relocation_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), n,
                     opacities, scales, ratios, new_opacities, new_scales);
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}
