// ggd_blend_math.h -- the device expressions that decide whether a (pixel, record) pair contributes, and with which alpha, stated
// ONCE for every kernel that walks a tile's list: the colour blend (ggd_blend.hip) and, through ggd_quarter_walk.h, the passes
// that blend another map behind it (ggd_features.hip, which also carries the normals, and ggd_distortion.hip).  These are the
// leaf expressions; the sequence that combines them into a pair's contribution decision is bwd_update / the forward loop in
// ggd_blend.hip, pair_forward in ggd_quarter_walk.h and the backward kernels of the two passes.  With -ffp-contract=off the same
// expression gives the same bits in every translation unit, so a pass that recomputes alpha takes the colour pass's decision on
// every pair (the forward and the backward of the colour blend stay in step the same way).
// Included inside each file's unnamed namespace: the definitions keep internal linkage.
#pragma once

constexpr float ALPHA_FLOOR = 1.0f / 255.0f;

// exp() variants for the blend (GGD_OPT_EXP_MODE).
// The bare hardware exponential, written out: ONE expression shared by the forward (mode 1, and the forward half of the default
// mode 3) and by the backward's contribution decision (bwd_update<3>), so that the two passes cannot drift apart with the way a
// ROCm release lowers __expf: v_exp_f32(fl(x * log2e)), ~3 ulp on [-6, 0].
constexpr float BLEND_LOG2E = 1.44269502162933349609375f;
__device__ __forceinline__ float blend_exp_bare(float x) { return __builtin_amdgcn_exp2f(x * BLEND_LOG2E); }

template <int MODE>
__device__ __forceinline__ float blend_exp(float x) {
  if (MODE == 1) return blend_exp_bare(x);
  if (MODE == 2) {                  // 2^(hi) * (1 + lo*ln2): hi = fl(x*log2e), lo = exact product residual + low bits
    const float t = x * 1.44269502162933349609375f;
    float lo = __builtin_fmaf(x, 1.44269502162933349609375f, -t);
    lo = __builtin_fmaf(x, 1.925963033500011e-08f, lo);
    const float e = __builtin_amdgcn_exp2f(t);
    return __builtin_fmaf(e, lo * 0.693147182464599609375f, e);
  }
  return expf(x);                   // ocml, <= 1 ulp
}

// `power` of a pixel at (px, py) under a staged record {x, y, hA, nB | hC ...}: operation order == the published form
__device__ __forceinline__ float blend_power(float x, float y, float hA, float nB, float hC, float px, float py, float& dx,
                                             float& dy) {
  dy = y - py;
  const float nBdy = nB * dy, hCdy2 = (hC * dy) * dy;
  dx = x - px;
  return __builtin_fmaf(__builtin_fmaf(hA, dx, nBdy), dx, hCdy2);
}

// The backward's exponential for a mode: g0 = the value the derivatives use, adec = the alpha the contribution decision is taken
// on.  Mode 3 (the default pairing: bare v_exp_f32 in the forward, compensated 2^x in the backward) decides on the forward's own
// number -- e below is exactly the forward's G -- while the values use the compensated exponential; every other mode decides on
// the value it differentiates.
template <int EXP_MODE>
__device__ __forceinline__ float blend_exp_backward(float pw, float opacity, float& adec) {
  float g0;
  if constexpr (EXP_MODE == 3) {
    const float t = pw * BLEND_LOG2E;
    float lo = __builtin_fmaf(pw, BLEND_LOG2E, -t);
    lo = __builtin_fmaf(pw, 1.925963033500011e-08f, lo);
    const float e = blend_exp_bare(pw);          // == the forward's G, by construction (the compiler shares the product t)
    adec = fminf(0.99f, e * opacity);
    g0 = __builtin_fmaf(e, lo * 0.693147182464599609375f, e);
  } else {
    g0 = blend_exp<EXP_MODE>(pw);
    adec = fminf(0.99f, opacity * g0);
  }
  return g0;
}

// Record-level pre-cull, done ONCE per gathered record by the lane that gathers it (the per-pixel cull costs every lane
// of the wave ~13 issue slots per record): ggd_splat carries the half extents (ex, ey) of the axis-aligned box outside
// of which power < thr, i.e. alpha < 1/255 (formed once per Gaussian by the preprocess kernel, with the fp32 safety
// margins described there).  If that box misses the wave's pixel rectangle no pixel can pass the `power >= thr` test, so
// the record is never written to LDS.  Comparisons with +inf (indefinite conic: always kept) / -inf (opacity < 1/255:
// never kept) extents do the right thing.
__device__ __forceinline__ bool record_box_hits(float x, float y, float ex, float ey, float wx0, float wx1, float wy0,
                                                float wy1) {
  return !(x + ex < wx0 || x - ex > wx1 || y + ey < wy0 || y - ey > wy1);
}

// Second, exact stage of the pre-cull (same lane, only for records whose box hit): the largest `power` any point of the
// wave's pixel rectangle can reach.  power(d) = hA dx^2 + nB dx dy + hC dy^2 (d = centre - pixel) is concave for a
// positive-definite conic, so its maximum over the rectangle [dx0, dx1] x [dy0, dy1] is 0 if the rectangle contains the
// centre and otherwise sits on an edge facing the centre, where it is a 1-D parabola maximised at the clamped vertex.  An
// elongated, tilted splat whose bounding box clips a block's corner is dropped here instead of costing every lane of
// the wave a `power` evaluation.  Conservative: the test allows for the fp32 rounding of both evaluations (margin
// proportional to the magnitude of the three terms); non-positive-definite conics (ex = +inf) are always kept.
__device__ __forceinline__ bool record_reaches_block(float x, float y, float hA, float nB, float hC, float thr, float ex,
                                                     float wx0, float wx1, float wy0, float wy1) {
  if (!(ex < __builtin_huge_valf())) return true;
  const float dx0 = x - wx1, dx1 = x - wx0, dy0 = y - wy1, dy1 = y - wy0;
  if (dx0 <= 0.0f && dx1 >= 0.0f && dy0 <= 0.0f && dy1 >= 0.0f) return true;
  // vertex of the edge parabolas: dy* = -nB X / (2 hC), dx* = -nB Y / (2 hA).  (v_rcp_f32, 1 ulp: the correctly rounded
  // divisions the build flags ask for cost two dozen instructions per record here, and the margin below dwarfs an ulp)
  const float ihC = -0.5f * __builtin_amdgcn_rcpf(hC), ihA = -0.5f * __builtin_amdgcn_rcpf(hA);
  // A concave function grows along every segment towards its maximiser (the centre, outside the rectangle here), so its
  // maximum over the rectangle sits on an edge that FACES the centre: at most one edge per axis, the one nearer to it.
  const bool in_x = dx0 <= 0.0f && dx1 >= 0.0f, in_y = dy0 <= 0.0f && dy1 >= 0.0f;
  const float X = dx0 > 0.0f ? dx0 : dx1, Y = dy0 > 0.0f ? dy0 : dy1;
  const float dyv = fminf(fmaxf((nB * X) * ihC, dy0), dy1);
  const float t1 = hA * X * X, t2 = nB * X * dyv, t3 = hC * dyv * dyv;
  const float px_ = (t1 + t2) + t3, mx_ = (fabsf(t1) + fabsf(t2)) + fabsf(t3);
  const float dxv = fminf(fmaxf((nB * Y) * ihA, dx0), dx1);
  const float u1 = hA * dxv * dxv, u2 = nB * dxv * Y, u3 = hC * Y * Y;
  const float py_ = (u1 + u2) + u3, my_ = (fabsf(u1) + fabsf(u2)) + fabsf(u3);
  const float pmax = in_x ? py_ : (in_y ? px_ : fmaxf(px_, py_));
  const float mag = in_x ? my_ : (in_y ? mx_ : fmaxf(mx_, my_));
  return !(pmax < thr - (1e-3f + 1e-5f * mag));
}

// Workgroup -> tile placement of the blend kernels (speed only; any placement is correct).  Workgroup b runs on XCD
// b % 8 and every XCD has its own 4 MB L2: the nsub sub-blocks of one tile take consecutive slots of ONE XCD's dispatch
// stream (b = 8 q + x: slot q of XCD x), so they are resident together and all but the first gather of a record hit
// that L2 (measured, 4 waves per tile: FETCH_SIZE 178 -> 46 MB per frame, 156 -> 149 us; with the sub-blocks T
// workgroups apart the later ones re-fetched every record from the Infinity Cache).  Walking 8x8-tile patches per XCD
// on top of that halves the fetches again (23 MB) but costs time (151 us; shell 335 -> 354 us): neighbouring tiles
// finish together and leave the XCDs unevenly loaded -- not used.  Tile counts that are not multiples of 8 keep
// tile = b % T.
__device__ __forceinline__ void ggd_block_to_tile(int b, int nsub, int T, int& tile, int& sub) {
  if ((T & 7) == 0) { const int q = b >> 3; sub = q % nsub; tile = (q / nsub) * 8 + (b & 7); }
  else { tile = b % T; sub = b / T; }
}

// one (record, component) of the backward's flush: v = the component's reduced sum (for the two mean components the pair of
// sums), comp in accumulator-record order (conic A B C | opacity | mean x y | colour r g b)
__device__ __forceinline__ float bwd_scale(int comp, float v, float swx, float swy, float hA, float nB, float hC, float op,
                                           float ddelx_dx, float ddely_dy) {
  // d alpha / d G = opacity; d G / d conic = -1/2 G d d^T; d G / d mean = -G * conic * d, conic = (-2 hA, -nB, -2 hC)
  if (comp < 3) return (-0.5f * op) * v;
  if (comp == 4) return (op * ddelx_dx) * __builtin_fmaf(2.0f * hA, swx, nB * swy);
  if (comp == 5) return (op * ddely_dy) * __builtin_fmaf(2.0f * hC, swy, nB * swx);
  return v;
}
