// ggd_quarter_walk.h -- what the passes that walk a tile's list behind a finished colour render share (ggd_features.hip,
// ggd_distortion.hip): the placement of a single-wave workgroup on an 8x8 quarter of a tile and the two-stage gather of the
// list's records.  Included inside each file's unnamed namespace, behind ggd_blend_math.h.
#pragma once

constexpr int ROUND = GGD_FEATURES_ROUND;   // list entries gathered per round (one per lane)
static_assert(ROUND == 64, "a round is one list entry per lane");

// the wave's quarter and the lane's pixel
struct FeatGeom {
  int px, py, qx0, qy0;
  uint32_t lo, hi;
  bool in;
  size_t pix;
  __device__ __forceinline__ FeatGeom(int b, int W, int H, int gx, int T, const uint32_t* __restrict__ ranges, uint32_t R) {
    int tile, sub;
    ggd_block_to_tile(b, 4, T, tile, sub);
    const int tx = tile % gx, ty = tile / gx;
    const int lane = threadIdx.x;
    qx0 = tx * 16 + (sub & 1) * 8; qy0 = ty * 16 + (sub >> 1) * 8;
    px = qx0 + (lane & 7); py = qy0 + (lane >> 3);
    in = py < H && px < W;
    pix = (size_t)py * W + px;
    const uint2 r = reinterpret_cast<const uint2*>(ranges)[tile];
    lo = min(r.x, R); hi = min(r.y, R);
    if (hi < lo) hi = lo;
  }
};

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The gather of a round is the colour kernels' two-stage software pipeline: the list entries of round k + 2 and the 48-byte
// records of round k + 1 are requested (from clamped positions: unconditional loads, a lane past the round's end re-reads a valid
// entry and its record is never consumed) while round k is blended.
struct Gather {
  const ggd_splat* splat; const uint32_t* list;
  uint32_t lo, last_pos;                 // the tile's first list position / the last one this quarter walks
  uint32_t id_cur = 0, id_nxt = 0;       // Gaussian of the record in r0 .. r2 / list entry of the round after it
  float4 r0, r1, r2;                     // x y hA nB | hC thr opacity r | g b ex ey
  __device__ __forceinline__ void load_id(uint32_t pos0) { id_nxt = list[min(lo + pos0 + (uint32_t)threadIdx.x, last_pos)]; }
  __device__ __forceinline__ void load_rec() {
    id_cur = id_nxt;
    const float4* p = reinterpret_cast<const float4*>(splat + id_nxt);
    r0 = p[0]; r1 = p[1]; r2 = p[2];
  }
};
