// ggd_knn.hip -- exact 3-nearest-neighbour search over a point cloud: the `distCUDA2` of the simple_knn module that
// gaussian_splatting/scene/gaussian_model.py imports (:20) and create_from_pcd / create_from_pos_col call (:132, :160)
// to seed every Gaussian's scale with log(sqrt(mean squared distance to its three nearest other points)).
//
// The published algorithm, restated for wave64 / LDS:
//   box     bounding box of the cloud (two-step min/max reduction, no float atomics)
//   codes   30-bit Morton code of every point inside that box
//   sort    (code, index) by the library's own onesweep radix sort (ggd_binning.hip, 32-bit keys, identity values)
//   leaves  points gathered into sorted order as float4 (x, y, z, original index); one box per leaf of KNN_L = 64
//           consecutive sorted points
//   search  ONE WORKGROUP PER 256 CONSECUTIVE QUERIES (four leaves), one query per lane.  A wave's own leaf (in LDS)
//           seeds each query's three best; then all leaf boxes are tested cooperatively, 256 at a time and outward from
//           the group's own position, against the group's query boxes and its largest third-best distances; the
//           survivors are tested per query, and those somebody needs are staged through LDS KNN_BATCH at a time
//           (coalesced float4 loads shared by the whole group); every query re-tests a leaf's box against its OWN
//           third-best before it scans the leaf's points (LDS broadcast reads, eight candidates per step).
//
// Arithmetic contract (tests compare bit for bit with a numpy fp32 brute force): d = (dx*dx + dy*dy) + dz*dz with
// dx = a.x - b.x, no contraction (-ffp-contract=off); the three smallest d over all OTHER indices ascending b0 <= b1 <= b2;
// result ((b0 + b1) + b2) / 3.0f, division correctly rounded.  Pruning is value-safe: the per-axis gap
// max(0, lo - p, p - hi) is, by monotonicity of fp32 rounding, never larger than |p - c| computed in fp32 for any c in
// the box, and squares / sums in the same order keep that; the box-to-box gap bounds every query of the group the same
// way.  A leaf is pruned when its bound is >= the current third-best, so coincident points stop after one leaf.
// Every loop is bounded by P and the leaf count whatever the coordinates hold (NaN compares false: never inserted,
// never pruned by accident into an endless loop -- there is none).
#include "ggd_common.h"

#include <math.h>

namespace {

constexpr int KNN_L = 64;           // points per leaf: one wave of queries, and the unit of pruning
constexpr int KNN_T = 256;          // threads per workgroup = queries per workgroup (KNN_WAVES consecutive leaves)
constexpr int KNN_WAVES = KNN_T / GGD_WAVE;
constexpr int KNN_BATCH = 16;       // leaves staged in LDS between two barriers (16 x 1 KiB)
constexpr int KNN_BOX_WGS = 256;    // partial boxes of the first reduction step
constexpr int32_t KNN_MAX_POINTS = 1 << 26;

// min / max over the workgroup of three lows and three highs; result valid in every thread.  red: 6 * KNN_WAVES floats.
__device__ __forceinline__ void knn_wg_minmax(float (&lo)[3], float (&hi)[3], float* red) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], m, GGD_WAVE));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m, GGD_WAVE));
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { red[wave * 6 + k] = lo[k]; red[wave * 6 + 3 + k] = hi[k]; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = red[k]; hi[k] = red[3 + k];
#pragma unroll
    for (int w = 1; w < KNN_WAVES; ++w) { lo[k] = fminf(lo[k], red[w * 6 + k]); hi[k] = fmaxf(hi[k], red[w * 6 + 3 + k]); }
  }
  __syncthreads();
}

// step 1 of the cloud's box: workgroup g reduces points g, g + G, ... (in rows of 256) into part[g] = {lo.xyz, -, hi.xyz, -}
__global__ __launch_bounds__(KNN_T) void knn_box_kernel(const float* __restrict__ pts, int P, float4* __restrict__ part) {
  __shared__ float red[6 * KNN_WAVES];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * KNN_T + threadIdx.x; i < P; i += (int64_t)gridDim.x * KNN_T) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float v = pts[3 * i + k]; lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); }
  }
  knn_wg_minmax(lo, hi, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    part[2 * blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

__device__ __forceinline__ uint32_t knn_spread10(uint32_t v) {   // 10 bits -> every third bit of 30
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// step 2 of the box (every workgroup folds the nparts partial boxes again: 8 KiB out of L2) + the Morton codes.
// The code only orders the points; any value is a valid one, so non-finite input just lands at cell 0.
__global__ __launch_bounds__(KNN_T) void knn_codes_kernel(const float* __restrict__ pts, int P, const float4* __restrict__ part,
                                                          int nparts, uint32_t* __restrict__ codes) {
  __shared__ float red[6 * KNN_WAVES];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if ((int)threadIdx.x < nparts) {
    const float4 a = part[2 * threadIdx.x], b = part[2 * threadIdx.x + 1];
    lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
  }
  knn_wg_minmax(lo, hi, red);
  const int64_t i = (int64_t)blockIdx.x * KNN_T + threadIdx.x;
  if (i >= P) return;
  uint32_t code = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float ext = hi[k] - lo[k];
    const float inv = ext > 0.0f ? 1023.0f / ext : 0.0f;
    const int c = min(1023, max(0, (int)((pts[3 * i + k] - lo[k]) * inv)));   // float -> int saturates, NaN -> 0
    code |= knn_spread10((uint32_t)c) << (2 - k);
  }
  codes[i] = code;
}

// gather into sorted order + one box per leaf (lo.xyz | hi.xyz, the fourth lanes unused): a leaf is a wave here
__global__ __launch_bounds__(KNN_T) void knn_leaves_kernel(const float* __restrict__ pts, const uint32_t* __restrict__ order, int P,
                                                           float4* __restrict__ sp, float4* __restrict__ leaf_lo,
                                                           float4* __restrict__ leaf_hi) {
  static_assert(KNN_L == GGD_WAVE, "one leaf per wave");
  const int64_t i = (int64_t)blockIdx.x * KNN_T + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < P) {
    uint32_t o = order[i];
    if (o >= (uint32_t)P) o = 0;   // cannot happen (the sort permutes 0..P-1); keeps the gather in bounds regardless
    const float x = pts[3 * (size_t)o], y = pts[3 * (size_t)o + 1], z = pts[3 * (size_t)o + 2];
    sp[i] = make_float4(x, y, z, __uint_as_float(o));
    lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], m, GGD_WAVE));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m, GGD_WAVE));
    }
  }
  const int64_t leaf = i / KNN_L;
  if ((threadIdx.x & 63) == 0 && leaf * KNN_L < P) {
    leaf_lo[leaf] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    leaf_hi[leaf] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

__device__ __forceinline__ float knn_gap(float lo, float hi, float qlo, float qhi) {
  return fmaxf(0.0f, fmaxf(lo - qhi, qlo - hi));
}

struct Best3 { float d0, d1, d2; uint32_t i0, i1, i2; };

__device__ __forceinline__ float knn_dist2(const float4 q, const float4 c) {
  const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ void knn_insert(Best3& b, float d, uint32_t ci) {
  if (d < b.d2) {
    if (d < b.d1) {
      b.d2 = b.d1; b.i2 = b.i1;
      if (d < b.d0) { b.d1 = b.d0; b.i1 = b.i0; b.d0 = d; b.i0 = ci; }
      else { b.d1 = d; b.i1 = ci; }
    } else { b.d2 = d; b.i2 = ci; }
  }
}

// One staged leaf (KNN_L float4 in LDS, the slots behind a short leaf hold +inf coordinates: their distance is +inf or NaN
// and never enters) against one query, KNN_UNROLL candidates per step: the LDS reads (all lanes one address: a broadcast)
// and the distances of a step are independent, and only a step whose smallest distance beats the third-best walks the
// insertion.  skip: the slot of the query itself in its own leaf (-1: none).
constexpr int KNN_UNROLL = 8;
__device__ __forceinline__ void knn_scan_leaf(Best3& b, const float4 q, const float4* __restrict__ cp, int skip) {
  for (int c = 0; c < KNN_L; c += KNN_UNROLL) {
    float4 p[KNN_UNROLL];
    float d[KNN_UNROLL];
#pragma unroll
    for (int u = 0; u < KNN_UNROLL; ++u) p[u] = cp[c + u];
#pragma unroll
    for (int u = 0; u < KNN_UNROLL; ++u) {
      d[u] = knn_dist2(q, p[u]);
      if (c + u == skip) d[u] = INFINITY;
    }
    float dm = d[0];
#pragma unroll
    for (int u = 1; u < KNN_UNROLL; ++u) dm = fminf(dm, d[u]);
    if (dm < b.d2) {
#pragma unroll
      for (int u = 0; u < KNN_UNROLL; ++u) knn_insert(b, d[u], __float_as_uint(p[u].w));
    }
  }
}

__device__ __forceinline__ float knn_wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, GGD_WAVE));
  return v;
}

__device__ __forceinline__ float knn_point_box(const float4 q, const float4 lo, const float4 hi) {
  const float gx = fmaxf(0.0f, fmaxf(lo.x - q.x, q.x - hi.x)), gy = fmaxf(0.0f, fmaxf(lo.y - q.y, q.y - hi.y)),
              gz = fmaxf(0.0f, fmaxf(lo.z - q.z, q.z - hi.z));
  return (gx * gx + gy * gy) + gz * gz;
}

// COUNT: the instance that also sums the number of evaluated candidates (ggd_knn3's `examined`); the plain one has no
// trace of it.
//
// A workgroup owns KNN_T Morton-consecutive queries = KNN_WAVES leaves, one query per lane, wave w = leaf w of the group.
// Seed: the wave's own leaf.  Then, per chunk of 256 leaves: (1) every lane tests one leaf box against the group's two
// query boxes and their radii (the largest third-best on each side) -- most chunks end here, after one barrier; (2) the
// survivors go to an LDS list, boxes included, and every query tests them against its own third-best: a leaf nobody needs
// is never staged; (3) the needed leaves are staged KNN_BATCH at a time -- coalesced float4 loads, shared by the group --
// and every query re-tests a leaf's box before it scans the leaf.
template <bool COUNT>
__global__ __launch_bounds__(KNN_T) void knn_search_kernel(const float4* __restrict__ sp, const float4* __restrict__ leaf_lo,
                                                           const float4* __restrict__ leaf_hi, int P, int nleaves,
                                                           float* __restrict__ mean_out, float* __restrict__ dist_out,
                                                           int32_t* __restrict__ idx_out, unsigned long long* __restrict__ examined) {
  __shared__ float4 s_pts[KNN_BATCH * KNN_L];
  __shared__ float4 s_hlo[KNN_T], s_hhi[KNN_T];
  __shared__ int s_leaf[KNN_T];
  __shared__ int s_sel[KNN_T];
  __shared__ int s_need[KNN_T];
  __shared__ int s_wcnt[2][KNN_WAVES];
  __shared__ int s_wcnt2[KNN_WAVES];
  __shared__ float s_wmax[2][KNN_WAVES];
  __shared__ unsigned long long s_wgap[KNN_WAVES];
  __shared__ float s_red[6 * KNN_WAVES];
  static_assert(KNN_WAVES == 4 && KNN_L == GGD_WAVE && KNN_BATCH * KNN_L >= KNN_T && KNN_BATCH % KNN_WAVES == 0, "layout");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int base = blockIdx.x * KNN_T;
  const int myleaf = blockIdx.x * KNN_WAVES + wave;
  const bool active = base + tid < P;
  const float4 pad = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
  float4 q = pad;   // an idle lane: every test it makes compares false
  if (active) q = sp[base + tid];
  s_pts[tid] = q;
  __syncthreads();
  Best3 b = {INFINITY, INFINITY, INFINITY, 0u, 0u, 0u};
  unsigned long long cnt = 0;
  // seed: the query's own leaf, every point but itself (a different index: coincident points count)
  if (active) {
    knn_scan_leaf(b, q, s_pts + wave * KNN_L, lane);
    if (COUNT) cnt += (unsigned)(min(KNN_L, P - myleaf * KNN_L) - 1);
  }
  // The group's queries as TWO boxes, cut at the largest step between consecutive queries: a run of the Morton order that
  // crosses a high-level cell boundary jumps across the cloud there, and one box around it would touch every leaf.
  unsigned long long gk = 0;
  if (base + tid + 1 < P && tid + 1 < KNN_T)
    gk = ((unsigned long long)__float_as_uint(knn_dist2(q, s_pts[tid + 1])) << 32) | (unsigned)(KNN_T - 1 - tid);
#pragma unroll
  for (int mm = 32; mm >= 1; mm >>= 1) { const unsigned long long o = __shfl_xor(gk, mm, GGD_WAVE); gk = o > gk ? o : gk; }
  if (lane == 0) s_wgap[wave] = gk;
  __syncthreads();   // also: everybody is done with the seed's s_pts
#pragma unroll
  for (int w = 0; w < KNN_WAVES; ++w) gk = s_wgap[w] > gk ? s_wgap[w] : gk;
  const int split = gk ? KNN_T - (int)(gk & 0xFFFFFFFFu) : KNN_T;   // queries [0, split) | [split, KNN_T)
  const bool in_a = tid < split;
  float4 alo, ahi, blo, bhi;
  {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (active && in_a) { lo[0] = hi[0] = q.x; lo[1] = hi[1] = q.y; lo[2] = hi[2] = q.z; }
    knn_wg_minmax(lo, hi, s_red);
    alo = make_float4(lo[0], lo[1], lo[2], 0.0f); ahi = make_float4(hi[0], hi[1], hi[2], 0.0f);
    float lo2[3] = {INFINITY, INFINITY, INFINITY}, hi2[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (active && !in_a) { lo2[0] = hi2[0] = q.x; lo2[1] = hi2[1] = q.y; lo2[2] = hi2[2] = q.z; }
    knn_wg_minmax(lo2, hi2, s_red);
    blo = make_float4(lo2[0], lo2[1], lo2[2], 0.0f); bhi = make_float4(hi2[0], hi2[1], hi2[2], 0.0f);
  }
  // an idle lane's radius is 0: it never raises a group radius and fails every leaf test
  float r = active ? b.d2 : 0.0f;
  // group radii: the largest third-best on either side of the cut
  float RA, RB;
#define KNN_PUBLISH_RADII()                                            \
  {                                                                    \
    const float wa = knn_wave_max(in_a ? r : 0.0f), wb = knn_wave_max(in_a ? 0.0f : r); \
    if (lane == 0) { s_wmax[0][wave] = wa; s_wmax[1][wave] = wb; }     \
  }
#define KNN_READ_RADII()                                                                              \
  RA = fmaxf(fmaxf(s_wmax[0][0], s_wmax[0][1]), fmaxf(s_wmax[0][2], s_wmax[0][3]));                   \
  RB = fmaxf(fmaxf(s_wmax[1][0], s_wmax[1][1]), fmaxf(s_wmax[1][2], s_wmax[1][3]));
  KNN_PUBLISH_RADII();
  __syncthreads();
  KNN_READ_RADII();

  // chunks of 256 leaves, outward from the group's own chunk (its Morton neighbours first: they tighten the radii most)
  const int nchunks = (nleaves + KNN_T - 1) / KNN_T;
  int up = (blockIdx.x * KNN_WAVES) / KNN_T, dn = up - 1;
  bool turn_up = true;
  auto next_chunk = [&]() -> int {
    if (up >= nchunks && dn < 0) return -1;
    const bool take_up = up < nchunks && (turn_up || dn < 0);
    turn_up = !take_up;
    return take_up ? up++ : dn--;
  };
  int cur = next_chunk();
  float4 nlo = pad, nhi = pad;
  if (cur * KNN_T + tid < nleaves) { nlo = leaf_lo[cur * KNN_T + tid]; nhi = leaf_hi[cur * KNN_T + tid]; }
  int par = 0;
  for (; cur >= 0; par ^= 1) {
    const int j = cur * KNN_T + tid;
    const float4 lo = nlo, hi = nhi;
    cur = next_chunk();
    if (cur >= 0 && cur * KNN_T + tid < nleaves) { nlo = leaf_lo[cur * KNN_T + tid]; nhi = leaf_hi[cur * KNN_T + tid]; }   // a round ahead
    bool hit = false;
    if (j < nleaves) {
      const float ax = knn_gap(lo.x, hi.x, alo.x, ahi.x), ay = knn_gap(lo.y, hi.y, alo.y, ahi.y),
                  az = knn_gap(lo.z, hi.z, alo.z, ahi.z);
      const float bx = knn_gap(lo.x, hi.x, blo.x, bhi.x), by = knn_gap(lo.y, hi.y, blo.y, bhi.y),
                  bz = knn_gap(lo.z, hi.z, blo.z, bhi.z);
      hit = (ax * ax + ay * ay) + az * az < RA || (bx * bx + by * by) + bz * bz < RB;
    }
    // survivors in leaf order (deterministic): ballot rank inside the wave, wave counts through LDS (two sets used in
    // turn: a chunk without survivors costs ONE barrier)
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wcnt[par][wave] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < KNN_WAVES; ++w) { const int c = s_wcnt[par][w]; off += w < wave ? c : 0; total += c; }
    if (total == 0) continue;
    if (hit) {
      const int slot = off + __popcll(m & below);
      s_leaf[slot] = j; s_hlo[slot] = lo; s_hhi[slot] = hi;
    }
    s_need[tid] = 0;
    __syncthreads();
    // which survivors does at least one query need?  (its own leaf is done: the seed)
    // (four list entries per step: independent LDS reads; entries past `total` are stale, and ignored below)
    for (int h0 = 0; h0 < total; h0 += 4) {
      bool want[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int h = (h0 + u) & (KNN_T - 1);
        want[u] = s_leaf[h] != myleaf && knn_point_box(q, s_hlo[h], s_hhi[h]) < r;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (__ballot(want[u]) != 0ull && lane == 0) s_need[(h0 + u) & (KNN_T - 1)] = 1;
    }
    __syncthreads();
    const bool keep = tid < total && s_need[tid] != 0;
    const unsigned long long m2 = __ballot(keep);
    if (lane == 0) s_wcnt2[wave] = __popcll(m2);
    __syncthreads();
    int off2 = 0, total2 = 0;
#pragma unroll
    for (int w = 0; w < KNN_WAVES; ++w) { const int c = s_wcnt2[w]; off2 += w < wave ? c : 0; total2 += c; }
    if (keep) s_sel[off2 + __popcll(m2 & below)] = tid;
    __syncthreads();
    for (int b0 = 0; b0 < total2; b0 += KNN_BATCH) {
      const int nb = min(KNN_BATCH, total2 - b0);
      for (int k = wave; k < nb; k += KNN_WAVES) {   // a wave stages a leaf
        const int cb = s_leaf[s_sel[b0 + k]] * KNN_L;
        float4 v = pad;
        if (lane < P - cb) v = sp[cb + lane];
        s_pts[k * KNN_L + lane] = v;
      }
      __syncthreads();
      for (int k = 0; k < nb; ++k) {
        const int h = s_sel[b0 + k];
        const int jl = s_leaf[h];
        if (jl != myleaf && knn_point_box(q, s_hlo[h], s_hhi[h]) < r) {
          knn_scan_leaf(b, q, s_pts + k * KNN_L, -1);
          if (COUNT) cnt += (unsigned)min(KNN_L, P - jl * KNN_L);
          r = b.d2;
        }
      }
      KNN_PUBLISH_RADII();
      __syncthreads();   // the batch's s_pts are free again, the wave maxima are published
      KNN_READ_RADII();
    }
  }
#undef KNN_PUBLISH_RADII
#undef KNN_READ_RADII

  if (active) {
    const uint32_t o = __float_as_uint(q.w);
    if (o < (uint32_t)P) {
      if (mean_out) mean_out[o] = ((b.d0 + b.d1) + b.d2) / 3.0f;
      if (dist_out) { dist_out[3 * (size_t)o] = b.d0; dist_out[3 * (size_t)o + 1] = b.d1; dist_out[3 * (size_t)o + 2] = b.d2; }
      if (idx_out) { idx_out[3 * (size_t)o] = (int32_t)b.i0; idx_out[3 * (size_t)o + 1] = (int32_t)b.i1; idx_out[3 * (size_t)o + 2] = (int32_t)b.i2; }
    }
  }
  if (COUNT) {
#pragma unroll
    for (int mm = 32; mm >= 1; mm >>= 1) cnt += __shfl_xor(cnt, mm, GGD_WAVE);
    if (lane == 0) atomicAdd(examined, cnt);
  }
}

struct KnnLayout {
  uint32_t *order, *codes, *ka, *kb, *vb;
  float4 *sp, *leaf_lo, *leaf_hi, *part;
  void* sort_tmp;
  size_t sort_bytes, total;
};

// [order (sorted indices) | codes, ka, kb, vb: the sort's buffers, REUSED as the gathered float4 points once the sort is
//  done | leaf boxes | partial boxes | sort control]
KnnLayout knn_layout(int32_t P, void* tmp) {
  KnnLayout v{};
  const size_t col = ggd_align((size_t)P * sizeof(uint32_t));
  const size_t leaves = ((size_t)P + KNN_L - 1) / KNN_L;
  char* p = static_cast<char*>(tmp);
  size_t o = 0;
  v.order = reinterpret_cast<uint32_t*>(p + o); o += col;
  v.sp = reinterpret_cast<float4*>(p + o);
  v.codes = reinterpret_cast<uint32_t*>(p + o); o += col;
  v.ka = reinterpret_cast<uint32_t*>(p + o); o += col;
  v.kb = reinterpret_cast<uint32_t*>(p + o); o += col;
  v.vb = reinterpret_cast<uint32_t*>(p + o); o += col;
  v.leaf_lo = reinterpret_cast<float4*>(p + o); o += ggd_align(leaves * sizeof(float4));
  v.leaf_hi = reinterpret_cast<float4*>(p + o); o += ggd_align(leaves * sizeof(float4));
  v.part = reinterpret_cast<float4*>(p + o); o += ggd_align((size_t)2 * KNN_BOX_WGS * sizeof(float4));
  v.sort_tmp = p + o; v.sort_bytes = ggd_sort32_tmp_bytes(P); o += ggd_align(v.sort_bytes);
  v.total = o;
  return v;
}

enum { KNN_ST_BOX = 1, KNN_ST_CODES = 2, KNN_ST_SORT = 4, KNN_ST_LEAVES = 8, KNN_ST_SEARCH = 16, KNN_ST_ALL = 31 };

int knn_run(ggd_ctx* ctx, void* stream, const float* points, int32_t P, float* mean_dist2, float* dist2, int32_t* idx,
            unsigned long long* examined, void* tmp, size_t tmp_bytes, int stages) {
  if (!ctx) return GGD_E_INVALID;
  if (P < 4 || P > KNN_MAX_POINTS) return ggd_fail(ctx, GGD_E_INVALID, "ggd_knn3: P must be in 4 .. 2^26");
  if (!points || !tmp) return ggd_fail(ctx, GGD_E_INVALID, "ggd_knn3: NULL pointer");
  if ((reinterpret_cast<uintptr_t>(tmp) & 15u) != 0) return ggd_fail(ctx, GGD_E_INVALID, "ggd_knn3: tmp must be 16-byte aligned");
  const KnnLayout v = knn_layout(P, tmp);
  if (tmp_bytes < v.total) return ggd_fail(ctx, GGD_E_INVALID, "ggd_knn3: tmp too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nleaves = (P + KNN_L - 1) / KNN_L;
  const int ngroups = (P + KNN_T - 1) / KNN_T;
  const int nparts = ngroups < KNN_BOX_WGS ? ngroups : KNN_BOX_WGS;
  if (stages & KNN_ST_BOX)
    hipLaunchKernelGGL(knn_box_kernel, dim3(nparts), dim3(KNN_T), 0, s, points, P, v.part);
  if (stages & KNN_ST_CODES)
    hipLaunchKernelGGL(knn_codes_kernel, dim3(ngroups), dim3(KNN_T), 0, s, points, P, v.part, nparts, v.codes);
  if (stages & KNN_ST_SORT) {
    // Morton codes are < 2^30, so no key equals the value (~0) that this sort drops; result in (ka, order)
    const int rc = ggd_launch_sort32_iota(ctx, s, v.codes, v.ka, v.order, v.kb, v.vb, P, 32, v.sort_tmp, v.sort_bytes);
    if (rc != GGD_OK) return rc;
  }
  if (stages & KNN_ST_LEAVES)
    hipLaunchKernelGGL(knn_leaves_kernel, dim3(ngroups), dim3(KNN_T), 0, s, points, v.order, P, v.sp, v.leaf_lo, v.leaf_hi);
  if (stages & KNN_ST_SEARCH) {
    if (examined)
      hipLaunchKernelGGL(knn_search_kernel<true>, dim3(ngroups), dim3(KNN_T), 0, s, v.sp, v.leaf_lo, v.leaf_hi, P, nleaves,
                         mean_dist2, dist2, idx, examined);
    else
      hipLaunchKernelGGL(knn_search_kernel<false>, dim3(ngroups), dim3(KNN_T), 0, s, v.sp, v.leaf_lo, v.leaf_hi, P, nleaves,
                         mean_dist2, dist2, idx, examined);
  }
  GGD_HIP(hipGetLastError());
  return GGD_OK;
}

}  // namespace

extern "C" size_t ggd_knn_tmp_bytes(int32_t P) {
  if (P < 4 || P > KNN_MAX_POINTS) return 0;
  return knn_layout(P, nullptr).total;
}

extern "C" int32_t ggd_knn_leaf_size(void) { return KNN_L; }

extern "C" int32_t ggd_knn_max_points(void) { return KNN_MAX_POINTS; }

extern "C" int ggd_knn3(ggd_ctx* ctx, void* stream, const float* points, int32_t P, float* mean_dist2, float* dist2,
                        int32_t* idx, unsigned long long* examined, void* tmp, size_t tmp_bytes) {
  return knn_run(ctx, stream, points, P, mean_dist2, dist2, idx, examined, tmp, tmp_bytes, KNN_ST_ALL);
}

extern "C" int ggd_knn3_stage(ggd_ctx* ctx, void* stream, const float* points, int32_t P, float* mean_dist2, float* dist2,
                              int32_t* idx, unsigned long long* examined, void* tmp, size_t tmp_bytes, int32_t stage) {
  if (stage < 0 || stage > 4) return ctx ? ggd_fail(ctx, GGD_E_INVALID, "ggd_knn3_stage: stage must be 0..4") : GGD_E_INVALID;
  return knn_run(ctx, stream, points, P, mean_dist2, dist2, idx, examined, tmp, tmp_bytes, 1 << stage);
}
