// ggd_triplane.hip -- tri-plane feature gather for the per-point decoder (the caller on the input side of the raster
// hot path; SURVEY.md section 8f row 1 "optionally fuse the tri-plane gather").
//
// Computes what the reference does with three torch ops (main/decoder_models/sequential_decoder_reverse.py:42-57 ->
// eg3d/training/volumetric_rendering/renderer.py:40-65 `sample_from_planes`, then `triplane_features.mean(0)` in
// main/decoder_models/base_decoder.py:22):   out[n, :] = (1/3) * sum_p bilinear(plane_p, proj_p(pos_n))
// with grid_sample semantics (bilinear, zero padding, align_corners = False) and the EG3D plane axes
// (plane 0 -> (x, y), plane 1 -> (x, z), plane 2 -> (z, x)).
//
// Layout: planes are CHANNEL-LAST [3][H][W][C] so that one texel's C channels are contiguous (C = 32 -> one 128-byte
// line): lane = channel, 64/C points per wave; every texel access is one coalesced line read, and the backward's
// scatter-add is one line-wide group of float atomics per texel (torch's NCHW grid_sampler_2d_backward issues one
// scattered atomic per (point, channel): 9.6 ms per 5e5 points measured on MI355X; this kernel is HBM/L2 bound).
//
// Kernels: plane_kernel<C, G3, BACKWARD> (lane = channel; the forward for C < 16, the backward for few points or C < 16),
// gather4_kernel<C, G3> (the forward for C >= 16), sr_keys_kernel<G3> + the library's sort + sr_accumulate_kernel<C, G3>
// (the backward for many points, C >= 16).  G3: tri-grids (D > 0).  The tap arithmetic of all of them is ggd_planes.h's.
#include "ggd_common.h"
#include "ggd_planes.h"

namespace {

bool channels_ok(int C) { return C > 0 && C <= 64 && (C & (C - 1)) == 0; }

// The runtime channel count as a compile-time constant: f(std::integral_constant<int, C>{}) for C in {1, 2, 4 .. 64};
// false, and f not called, for every other count.
template <typename F>
bool dispatch_channels(int C, F&& f) {
  if (!channels_ok(C)) return false;
  ggd_dispatch<7>(__builtin_ctz((unsigned)C), [&](auto lg) { f(std::integral_constant<int, 1 << decltype(lg)::value>{}); });
  return true;
}

// One kernel for both forms (G3 = false: planes [3][H][W][C], D unused; true: grids [3][D][H][W][C]) and both directions.
// Tri-grid: every "plane" is a C x D grid sampled with a 3-D grid_sample (trilinear, zero padding, align_corners = False) at
// the point's three projected coordinates (PanoHead/training/volumetric_rendering/renderer.py:47-58; selected at
// main/decoder_models/sequential_decoder_reverse.py:42-50).  mod: [C] (2-D) or [D][C], or null.
// Each form keeps its order of operations: forward w * (texel * m); 2-D backward w * ((dout / 3) * m), m taken once per lane;
// 3-D backward ((w * (dout / 3)) * m[z]).
template <int C, bool G3, bool BACKWARD>
__global__ __launch_bounds__(256) void plane_kernel(const float* __restrict__ grids_cl, float* __restrict__ dgrids_cl, int D,
                                                    int H, int W, int axes, const float* __restrict__ pos, int N, float scale,
                                                    const float* __restrict__ dout, float* __restrict__ out,
                                                    const float* __restrict__ mod) {
  constexpr int PPW = 64 / C;  // points per wave
  const int lane = threadIdx.x & 63;
  const int c = lane % C;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int64_t n = wave * PPW + lane / C;
  if (n >= N) return;
  const float x = scale * pos[3 * n], y = scale * pos[3 * n + 1], z = scale * pos[3 * n + 2];
  const size_t grid_stride = (size_t)(G3 ? D : 1) * H * W * C;
  float acc = 0.0f;
  // modulation (texel * m, rounded, is what is sampled): [C], taken once per lane (2-D), or [D][C], taken at the tap's slice
  const float m2 = (!G3 && mod) ? mod[c] : 1.0f;
  const float g = BACKWARD ? dout[n * C + c] * (1.0f / 3.0f) : 0.0f;
  const float gm2 = g * m2;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const PlaneCell cell = plane_cell<G3>(axes, p, x, y, z, D, H, W);
    const PlaneTap corner = cell_corner<G3>(cell);
#pragma unroll
    for (int k = 0; k < (G3 ? 8 : 4); ++k) {
      const PlaneTap tap = tap_at<G3>(corner, k);   // (used under the test only)
      // tap_in's three tests, written out: through the function they are evaluated without the branches between them, another
      // instruction stream than the tri-grid form of this kernel has had
      if (tap_inside(cell.fx, k & 1, W) && tap_inside(cell.fy, (k >> 1) & 1, H) && (!G3 || tap_inside(cell.fz, k >> 2, D))) {
        const float wgt = tap_weight<G3>(cell, k);
        const size_t off = p * grid_stride + tap_texel(tap, H, W) * C + c;
        const float m = !G3 ? m2 : mod ? mod[tap.z * C + c] : 1.0f;
        if (BACKWARD) atomicAdd(dgrids_cl + off, G3 ? wgt * g * m : wgt * gm2);
        else acc += wgt * (grids_cl[off] * m);
      }
    }
  }
  if (!BACKWARD) out[n * C + c] = acc * (1.0f / 3.0f);
}

// ---- the gather, four channels per lane (C a multiple of 4, C / 4 a power of two <= 16) -----------------------------------
// With lane = channel (the kernel above) the 64 / C points of a wave repeat the whole coordinate -> tap arithmetic in every
// one of their C lanes (~175 VALU instructions per point), and a 128-byte texel line costs a wave instruction per tap and
// point pair.  Here a point owns C / 4 lanes, each loading 16 bytes of a texel line: a wave holds 256 / C points (8 for
// C = 32), one global_load_dwordx4 instruction fetches one tap of all of them, and the arithmetic is repeated C / 4 times
// instead of C times.  Same operations per channel in the same order as the kernel above: bit-identical features.
// (Measured before the rewrite: visiting the points block by block of a 32^3 grid -- every line an L2 hit after its first
// use -- bought 35 of 336 us and cost a 50 us sort: the gather was bound by its own instruction stream, not by the fabric.)
template <int C, bool G3>
__global__ __launch_bounds__(256) void gather4_kernel(const float* __restrict__ grids_cl, int D, int H, int W, int axes,
                                                      const float* __restrict__ pos, int N, float scale,
                                                      float* __restrict__ out, const float* __restrict__ mod) {
  constexpr int LPP = C / 4;            // lanes per point
  constexpr int PPW = 64 / LPP;         // points per wave
  const int lane = threadIdx.x & 63;
  const int q = lane % LPP;             // which 16 bytes of a texel line
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int64_t n = wave * PPW + lane / LPP;
  if (n >= N) return;
  const float x = scale * pos[3 * n], y = scale * pos[3 * n + 1], z = scale * pos[3 * n + 2];
  const int Dd = G3 ? D : 1;
  const size_t grid_stride = (size_t)Dd * H * W * C;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const PlaneCell cell = plane_cell<G3>(axes, p, x, y, z, D, H, W);
    const PlaneTap corner = cell_corner<G3>(cell);
    // all taps of the plane are requested before the first is used
    float4 t[G3 ? 8 : 4];
    float wg[G3 ? 8 : 4];
    int zs[G3 ? 8 : 4];
#pragma unroll
    for (int k = 0; k < (G3 ? 8 : 4); ++k) {
      const PlaneTap tap = tap_at<G3>(corner, k);   // (used under `in` only; taken first: the order the stream depends on)
      const bool in = tap_in<G3>(cell, k, Dd, H, W);
      wg[k] = tap_weight<G3>(cell, k);
      zs[k] = in ? tap.z : -1;
      t[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (in) t[k] = *reinterpret_cast<const float4*>(grids_cl + p * grid_stride + tap_texel(tap, H, W) * C + 4 * q);
    }
#pragma unroll
    for (int k = 0; k < (G3 ? 8 : 4); ++k) {
      if (zs[k] >= 0) {   // (an outside tap adds nothing: skipped as the kernel above skips it, so that -0 / NaN texels cannot differ)
        float4 m = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        if (mod) m = *reinterpret_cast<const float4*>(mod + zs[k] * C + 4 * q);
        acc.x += wg[k] * (t[k].x * m.x); acc.y += wg[k] * (t[k].y * m.y);
        acc.z += wg[k] * (t[k].z * m.z); acc.w += wg[k] * (t[k].w * m.w);
      }
    }
  }
  const float third = 1.0f / 3.0f;
  *reinterpret_cast<float4*>(out + n * C + 4 * q) = make_float4(acc.x * third, acc.y * third, acc.z * third, acc.w * third);
}

template <int C>
int launch_gather4(ggd_ctx* ctx, hipStream_t s, const ggd_plane_set& ps, const float* pos, int N, float* out, const float* mod) {
  constexpr int PPW = 64 / (C / 4);
  const int64_t waves = ((int64_t)N + PPW - 1) / PPW;
  ggd_dispatch<2>(ps.D > 0, [&](auto g3) {
    hipLaunchKernelGGL((gather4_kernel<C, decltype(g3)::value != 0>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s,
                       ps.grids_cl, ps.D, ps.H, ps.W, ps.axes, pos, N, 2.0f / ps.box_warp, out, mod);
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

// the lane = channel kernel: forward (ps.grids_cl -> out) or backward (dout -> dgrids_cl)
template <int C, bool BACKWARD>
int launch_plane(ggd_ctx* ctx, hipStream_t s, const ggd_plane_set& ps, float* dgrids_cl, const float* pos, int N,
                 const float* dout, float* out, const float* mod) {
  const int64_t waves = ((int64_t)N + (64 / C) - 1) / (64 / C);
  ggd_dispatch<2>(ps.D > 0, [&](auto g3) {
    hipLaunchKernelGGL((plane_kernel<C, decltype(g3)::value != 0, BACKWARD>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s,
                       ps.grids_cl, dgrids_cl, ps.D, ps.H, ps.W, ps.axes, pos, N, 2.0f / ps.box_warp, dout, out, mod);
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Sorted-run backward (tri-planes AND tri-grids).  A training scene puts 5e5 surface points on a few 1e4 cells per plane:
// dozens of (point, plane) items per cell.  The items are sorted by cell (the library's 32-bit onesweep sort; items with
// no tap inside the grid carry the key ~0 and are dropped by its first pass), and a wave then walks a contiguous piece of
// the sorted list with the cell's 4 (8) tap sums in REGISTERS -- lane = channel, the 64 / C lane groups of a wave walk
// 64 / C disjoint sub-pieces -- and issues the taps' atomics once per run of equal cells.  No LDS accumulation tile (the
// 8 x 8-texel LDS tiles of the earlier design cost one dependent LDS read-add-write per item and tap and do not extend to
// a tri-grid: 9 x 9 x D x C floats per wave), global float atomics ~ cells x taps instead of items x taps.
constexpr int SR_CHUNK = 256;          // sorted items per wave
constexpr int SR_DEPTH = 8;            // gradient rows in flight per lane group
constexpr int SR_MOD_LDS = 1024;       // floats of the modulation table kept in LDS (D * C <= this; else read from memory)
constexpr int SR_MIN_POINTS = 49152;   // below: the plain scatter-add (the sort's launches cost more than they save)

struct SrGeom { int W, H, D, xb, yb, zb; };   // D = 0: 2-D planes; bit widths of the (x0 + 1), (y0 + 1), (z0 + 1) key fields
static inline int sr_bits(int vmax) { int b = 1; while ((1 << b) <= vmax) ++b; return b; }   // bits to hold 0 .. vmax

// cell key of item (point, plane p) -- plane | z0 + 1 | y0 + 1 | x0 + 1 -- and its interpolation fractions; ~0 when no tap
// lies inside the grid
template <bool G3>
__device__ __forceinline__ uint32_t sr_item(const SrGeom& g, int axes, int p, float x, float y, float z, float& ax, float& ay,
                                            float& az) {
  const PlaneCell c = plane_cell<G3>(axes, p, x, y, z, g.D, g.H, g.W);
  ax = c.ax(); ay = c.ay(); az = c.az();
  // does any tap lie inside?  On the float floors, false for NaN.  (Written out here: as a function of ggd_planes.h the same
  // lines compile sr_keys_kernel<true> to another instruction stream.)
  bool ok = c.fx >= -1.0f && c.fx <= (float)(g.W - 1) && c.fy >= -1.0f && c.fy <= (float)(g.H - 1);
  if (G3) ok = ok && c.fz >= -1.0f && c.fz <= (float)(g.D - 1);
  if (!ok) return ~0u;
  const PlaneTap corner = cell_corner<G3>(c);   // sound under the test above
  uint32_t key = (uint32_t)p;
  if (G3) key = (key << g.zb) | (uint32_t)(corner.z + 1);
  key = (key << g.yb) | (uint32_t)(corner.y + 1);
  key = (key << g.xb) | (uint32_t)(corner.x + 1);
  return key;
}

// the corner of a key's cell: the fields hold corner + 1 >= 0, so these integers are sound and may be range-tested
template <bool G3>
__device__ __forceinline__ PlaneTap sr_corner(const SrGeom& g, uint32_t key) {
  return PlaneTap{(int)(key & ((1u << g.xb) - 1u)) - 1, (int)((key >> g.xb) & ((1u << g.yb) - 1u)) - 1,
                  G3 ? (int)((key >> (g.xb + g.yb)) & ((1u << g.zb) - 1u)) - 1 : 0};
}

template <bool G3>
__global__ __launch_bounds__(256) void sr_keys_kernel(const float* __restrict__ pos, int N, float scale, SrGeom g, int axes,
                                                      uint32_t* __restrict__ keys /*[3][N]*/) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float x = scale * pos[3 * n], y = scale * pos[3 * n + 1], z = scale * pos[3 * n + 2];
  float ax, ay, az;
#pragma unroll
  for (int p = 0; p < 3; ++p) keys[(size_t)p * N + n] = sr_item<G3>(g, axes, p, x, y, z, ax, ay, az);
}

template <int C, bool G3>
__global__ __launch_bounds__(256) void sr_accumulate_kernel(
    const uint32_t* __restrict__ keys_a, const uint32_t* __restrict__ vals_a, const uint32_t* __restrict__ keys_b,
    const uint32_t* __restrict__ vals_b, const uint32_t* __restrict__ flat_flag, const uint32_t* __restrict__ n_valid_ptr,
    const float* __restrict__ pos, int N, float scale, SrGeom g, int axes, const float* __restrict__ dout,
    const float* __restrict__ mod, float* __restrict__ dgrid) {
  constexpr int G = 64 / C;            // lane groups = independent streams of one wave
  constexpr int T = G3 ? 8 : 4;
  constexpr int SL = SR_CHUNK / G;     // items per stream
  __shared__ uint4 s_rec[4][64];       // per item of the batch: point | run-start bit, ax, ay, az
  __shared__ uint32_t s_key[4][64];
  __shared__ float s_mod[SR_MOD_LDS];  // the modulation table: a flush must not wait on a global load (it would wait for
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;   // every gradient row in flight with it)
  const int nmod = (G3 ? g.D : 1) * C;
  const bool mod_lds = mod != nullptr && nmod <= SR_MOD_LDS;
  if (mod_lds) {
    for (int i = threadIdx.x; i < nmod; i += 256) s_mod[i] = mod[i];
    __syncthreads();
  }
  const uint32_t nv = *n_valid_ptr;
  const uint32_t wbase = (blockIdx.x * 4u + (uint32_t)wv) * SR_CHUNK;
  if (wbase >= nv) return;
  const bool flat = *flat_flag != 0u;  // the sort's last pass found a constant digit and left the result in (b)
  const uint32_t* keys = flat ? keys_b : keys_a;
  const uint32_t* vals = flat ? vals_b : vals_a;
  const int s = lane / C, c = lane % C;
  const uint32_t sbeg = wbase + (uint32_t)s * SL, send = min(nv, sbeg + SL);
  const int pshift = g.xb + g.yb + g.zb;
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.0f;
  uint32_t cur = ~0u;                  // the cell whose sums the lane group holds (~0: none)

  auto flush = [&](uint32_t key) {
    const PlaneTap corner = sr_corner<G3>(g, key);
    const int p = (int)(key >> pshift);
    const int Dd = G3 ? g.D : 1;
    float* base = dgrid + (size_t)p * Dd * g.H * g.W * C + c;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const PlaneTap tap = tap_at<G3>(corner, t);
      if (tap.x >= 0 && tap.x < g.W && tap.y >= 0 && tap.y < g.H && tap.z >= 0 && tap.z < Dd) {
        float v = acc[t] * (1.0f / 3.0f);
        if (mod_lds) v *= s_mod[tap.z * C + c];
        else if (mod) v *= mod[tap.z * C + c];
        atomicAdd(base + tap_texel(tap, g.H, g.W) * C, v);
      }
    }
  };

  for (uint32_t b0 = 0; b0 < (uint32_t)SL; b0 += C) {
    if (wbase + b0 >= nv) break;       // stream 0 is the earliest: nothing left for any stream
    {  // lane (s, c) prepares item c of its stream's batch
      const uint32_t i = sbeg + b0 + (uint32_t)c;
      uint32_t key = ~0u, rec0 = 0x80000000u;
      float ax = 0.0f, ay = 0.0f, az = 0.0f;
      if (i < send) {
        key = keys[i];
        const uint32_t prev = i > sbeg ? keys[i - 1] : ~0u;
        const uint32_t p = key >> pshift;
        const uint32_t n = vals[i] - p * (uint32_t)N;
        const float x = scale * pos[3 * (size_t)n], y = scale * pos[3 * (size_t)n + 1], z = scale * pos[3 * (size_t)n + 2];
        (void)sr_item<G3>(g, axes, (int)p, x, y, z, ax, ay, az);
        rec0 = n | ((i == sbeg || prev != key) ? 0x80000000u : 0u);
      }
      s_rec[wv][lane] = make_uint4(rec0, __builtin_bit_cast(uint32_t, ax), __builtin_bit_cast(uint32_t, ay),
                                   __builtin_bit_cast(uint32_t, az));
      s_key[wv][lane] = key;
    }
    __builtin_amdgcn_wave_barrier();
    for (int j0 = 0; j0 < C; j0 += SR_DEPTH) {
      uint4 r[SR_DEPTH];
      float gr[SR_DEPTH];
#pragma unroll
      for (int k = 0; k < SR_DEPTH; ++k) r[k] = s_rec[wv][s * C + j0 + k];
#pragma unroll
      for (int k = 0; k < SR_DEPTH; ++k) gr[k] = dout[(size_t)(r[k].x & 0x7fffffffu) * C + c];
#pragma unroll
      for (int k = 0; k < SR_DEPTH; ++k) {
        if (r[k].x >> 31) {            // first item of a run (uniform over the lane group): hand the finished cell over
          if (cur != ~0u) flush(cur);
          cur = s_key[wv][s * C + j0 + k];
#pragma unroll
          for (int t = 0; t < T; ++t) acc[t] = 0.0f;
        }
        const float ax = __builtin_bit_cast(float, r[k].y), ay = __builtin_bit_cast(float, r[k].z);
        const float bx = 1.0f - ax, by = 1.0f - ay;
        // weights in grid_sampler's order: (x) * (y) [* (z)]
        const float w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
        if constexpr (G3) {
          const float az = __builtin_bit_cast(float, r[k].w), bz = 1.0f - az;
          acc[0] = __builtin_fmaf(w00 * bz, gr[k], acc[0]); acc[1] = __builtin_fmaf(w10 * bz, gr[k], acc[1]);
          acc[2] = __builtin_fmaf(w01 * bz, gr[k], acc[2]); acc[3] = __builtin_fmaf(w11 * bz, gr[k], acc[3]);
          acc[4] = __builtin_fmaf(w00 * az, gr[k], acc[4]); acc[5] = __builtin_fmaf(w10 * az, gr[k], acc[5]);
          acc[6] = __builtin_fmaf(w01 * az, gr[k], acc[6]); acc[7] = __builtin_fmaf(w11 * az, gr[k], acc[7]);
        } else {
          acc[0] = __builtin_fmaf(w00, gr[k], acc[0]); acc[1] = __builtin_fmaf(w10, gr[k], acc[1]);
          acc[2] = __builtin_fmaf(w01, gr[k], acc[2]); acc[3] = __builtin_fmaf(w11, gr[k], acc[3]);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (cur != ~0u) flush(cur);
}

size_t sr_tmp_bytes(int N) {
  const size_t arr = ggd_align((size_t)3 * N * sizeof(uint32_t));
  return 5 * arr + ggd_sort32_tmp_bytes((int64_t)3 * N);
}

bool sr_supported(const ggd_plane_set& ps, int N) {
  if (ps.C < 16 || N < SR_MIN_POINTS || (int64_t)3 * N >= (1ll << 31)) return false;
  return 2 + sr_bits(ps.W) + sr_bits(ps.H) + (ps.D > 0 ? sr_bits(ps.D) : 0) <= 32;
}

template <int C>
int launch_sorted_backward(ggd_ctx* ctx, hipStream_t s, const ggd_plane_set& ps, const float* pos, int N, const float* dout,
                           const float* mod, float* dgrid) {
  int rc = ggd_reserve_scratch(ctx, sr_tmp_bytes(N), s);
  if (rc != GGD_OK) return rc;
  const float scale = 2.0f / ps.box_warp;
  const SrGeom g{ps.W, ps.H, ps.D, sr_bits(ps.W), sr_bits(ps.H), ps.D > 0 ? sr_bits(ps.D) : 0};
  const int64_t M = (int64_t)3 * N;
  const size_t arr = ggd_align((size_t)M * sizeof(uint32_t));
  char* p = static_cast<char*>(ctx->scratch);
  uint32_t* keys_src = reinterpret_cast<uint32_t*>(p); p += arr;
  uint32_t* keys_a = reinterpret_cast<uint32_t*>(p); p += arr;
  uint32_t* vals_a = reinterpret_cast<uint32_t*>(p); p += arr;
  uint32_t* keys_b = reinterpret_cast<uint32_t*>(p); p += arr;
  uint32_t* vals_b = reinterpret_cast<uint32_t*>(p); p += arr;
  void* sort_tmp = p;
  const size_t sort_bytes = ggd_sort32_tmp_bytes(M);
  ggd_dispatch<2>(ps.D > 0, [&](auto g3) {
    hipLaunchKernelGGL((sr_keys_kernel<decltype(g3)::value != 0>), dim3((N + 255) / 256), dim3(256), 0, s, pos, N, scale, g,
                       ps.axes, keys_src);
  });
  ggd_sort32_opts so;
  so.flag_flat_last = true;
  rc = ggd_launch_sort32_iota(ctx, s, keys_src, keys_a, vals_a, keys_b, vals_b, M, 32, sort_tmp, sort_bytes, so);
  if (rc != GGD_OK) return rc;
  const ggd_sort_ctl sc = ggd_sort_ctl::in_tmp(sort_tmp);
  const unsigned blocks = (unsigned)((M + 4 * SR_CHUNK - 1) / (4 * SR_CHUNK));
  ggd_dispatch<2>(ps.D > 0, [&](auto g3) {
    hipLaunchKernelGGL((sr_accumulate_kernel<C, decltype(g3)::value != 0>), dim3(blocks), dim3(256), 0, s, keys_a, vals_a, keys_b,
                       vals_b, sc.flat, sc.n_valid, pos, N, scale, g, ps.axes, dout, mod, dgrid);
  });
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

}  // namespace

extern "C" int ggd_planes_gather(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H,
                                 int32_t W, int32_t axes, const float* mod, const float* pos, int32_t N, float box_warp,
                                 float* out) {
  if (!ctx) return GGD_E_INVALID;
  const ggd_plane_set ps = {.grids_cl = grids_cl, .C = C, .D = D, .H = H, .W = W, .axes = axes, .box_warp = box_warp};
  int rc = ggd_check_plane_set(ctx, "ggd_planes_gather", ps);
  if (rc != GGD_OK) return rc;
  if (N > 0 && (!grids_cl || !pos || !out || H <= 0 || W <= 0 || box_warp == 0.0f))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_planes_gather: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (N <= 0) return GGD_OK;
  // four channels per lane where the channel count allows it (the decoder's 32); lane = channel otherwise
  const bool known = dispatch_channels(C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    if constexpr (CC >= 16) rc = launch_gather4<CC>(ctx, s, ps, pos, N, out, mod);
    else rc = launch_plane<CC, false>(ctx, s, ps, nullptr, pos, N, nullptr, out, mod);
  });
  if (!known)
    return ggd_fail(ctx, GGD_E_INVALID, std::string(D > 0 ? "trigrid" : "triplane") + ": channel count must be a power of two <= 64");
  return rc;
}

extern "C" int ggd_planes_scatter(ggd_ctx* ctx, void* stream, int32_t C, int32_t D, int32_t H, int32_t W, int32_t axes,
                                  const float* mod, const float* pos, int32_t N, float box_warp, const float* dout,
                                  float* dgrids_cl, int32_t accumulate) {
  if (!ctx) return GGD_E_INVALID;
  const ggd_plane_set ps = {.C = C, .D = D, .H = H, .W = W, .axes = axes, .box_warp = box_warp};   // the gradient buffer's shape
  if (!dgrids_cl || H <= 0 || W <= 0 || !ggd_plane_axes_ok(ps))   // (this entry has always said "bad argument" for the axes too)
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_planes_scatter: bad argument");
  if (!channels_ok(C))
    return ggd_fail(ctx, GGD_E_INVALID, "ggd_planes_scatter: channel count must be a power of two <= 64");
  // every refusal comes before the clear: a refused call leaves the caller's gradient buffer as it was
  if (N > 0 && (!pos || !dout || box_warp == 0.0f)) return ggd_fail(ctx, GGD_E_INVALID, "ggd_planes_scatter: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int Dd = D > 0 ? D : 1;
  if (!accumulate) GGD_HIP(hipMemsetAsync(dgrids_cl, 0, (size_t)3 * Dd * H * W * C * sizeof(float), s));
  if (N <= 0) return GGD_OK;
  // many points per cell: sort the (point, plane) items by cell and sum runs in registers; few: plain scatter-add
  const bool sorted = sr_supported(ps, N);
  int rc = GGD_OK;
  dispatch_channels(C, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    if constexpr (CC >= 16) {
      if (sorted) { rc = launch_sorted_backward<CC>(ctx, s, ps, pos, N, dout, mod, dgrids_cl); return; }
    }
    rc = launch_plane<CC, true>(ctx, s, ps, dgrids_cl, pos, N, dout, nullptr, mod);
  });
  return rc;
}

extern "C" int ggd_triplane_forward(ggd_ctx* ctx, void* stream, const float* planes_cl, int32_t C, int32_t H, int32_t W,
                                    const float* pos, int32_t N, float box_warp, float* out) {
  return ggd_planes_gather(ctx, stream, planes_cl, C, 0, H, W, 0, nullptr, pos, N, box_warp, out);
}

extern "C" int ggd_triplane_backward(ggd_ctx* ctx, void* stream, int32_t C, int32_t H, int32_t W, const float* pos,
                                     int32_t N, float box_warp, const float* dout, float* dplanes_cl) {
  return ggd_planes_scatter(ctx, stream, C, 0, H, W, 0, nullptr, pos, N, box_warp, dout, dplanes_cl, 0);
}

extern "C" int ggd_trigrid_forward(ggd_ctx* ctx, void* stream, const float* grids_cl, int32_t C, int32_t D, int32_t H,
                                   int32_t W, int32_t axes, const float* pos, int32_t N, float box_warp, float* out) {
  if (ctx && D <= 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_trigrid_forward: bad axes / depth");
  return ggd_planes_gather(ctx, stream, grids_cl, C, D, H, W, axes, nullptr, pos, N, box_warp, out);
}

extern "C" int ggd_trigrid_backward(ggd_ctx* ctx, void* stream, int32_t C, int32_t D, int32_t H, int32_t W, int32_t axes,
                                    const float* pos, int32_t N, float box_warp, const float* dout, float* dgrids_cl) {
  if (ctx && D <= 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_trigrid_backward: bad argument");
  return ggd_planes_scatter(ctx, stream, C, D, H, W, axes, nullptr, pos, N, box_warp, dout, dgrids_cl, 0);
}
