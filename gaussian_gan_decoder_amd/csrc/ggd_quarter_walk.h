// ggd_quarter_walk.h -- the walk of a tile's list behind a finished colour render, for the passes that blend another map over the
// colour pass's contributors (ggd_features.hip, ggd_distortion.hip): one single-wave workgroup per 8x8 quarter of a tile, one
// pixel per lane.  Stated ONCE here: the quarter and the pixel's contributor bound (QuarterGeom), the two-stage gather (Gather),
// the cull and compaction of a round (stage_cull), the forward step of a (pixel, record) pair with the colour kernels' skip tests
// in the colour kernels' order (pair_forward), the front-to-back round loop around it (walk_front), the backward's chunk
// constants and the launch prologue (quarter_launch).  A pass hands in what is its own as functors: what a round stages beyond
// the records, what a pair adds to the pixel's state.  The back-to-front walks stay written out in the two files: hoisted, their
// kernels measured slower; whoever changes the pair step there changes it in both, and in pair_forward.
// Included inside each file's unnamed namespace, behind ggd_blend_math.h.
#pragma once

constexpr int ROUND = GGD_FEATURES_ROUND;   // list entries gathered per round (one per lane)
static_assert(ROUND == 64, "a round is one list entry per lane");
constexpr int FLUSH = 32;                   // staged records per chunk of the backward (a record per lane pair in its flush)
constexpr int WPAD = 65;                    // row stride of the parked [record][pixel] matrices: lane = record reads without bank conflicts

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// the wave's quarter, the lane's pixel and its contributors: list positions 0 .. lastn - 1 of the tile; maxn: the largest lastn
// of the quarter, the entries its rounds walk
struct QuarterGeom {
  int px, py, qx0, qy0;
  uint32_t lo, hi, lastn, maxn;
  bool in;
  size_t pix;
  __device__ __forceinline__ QuarterGeom(int b, int W, int H, int gx, int T, const uint32_t* __restrict__ ranges, uint32_t R,
                                         const uint32_t* __restrict__ n_contrib) {
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
    lastn = in ? min(n_contrib[pix], hi - lo) : 0u;
    maxn = wave_max(lastn);
  }
};

// The gather of a round is the colour kernels' two-stage software pipeline: the list entries of round k + 2 and the 48-byte
// records of round k + 1 are requested (from clamped positions: unconditional loads, a lane past the round's end re-reads a valid
// entry and its record is never consumed) while round k is blended.
struct Gather {
  const ggd_splat* splat; const uint32_t* list;
  uint32_t lo, last_pos;                 // the tile's first list position / the last one this quarter walks
  uint32_t id_cur = 0, id_nxt = 0;       // Gaussian of the record in r0 .. r2 / list entry of the round after it
  float4 r0, r1, r2;                     // x y hA nB | hC thr opacity r | g b ex ey
  __device__ __forceinline__ Gather(const ggd_splat* splat_, const uint32_t* list_, const QuarterGeom& g)
      : splat(splat_), list(list_), lo(g.lo), last_pos(g.lo + g.maxn - 1u) {}
  __device__ __forceinline__ void load_id(uint32_t pos0) { id_nxt = list[min(lo + pos0 + (uint32_t)threadIdx.x, last_pos)]; }
  __device__ __forceinline__ void load_rec() {
    id_cur = id_nxt;
    const float4* p = reinterpret_cast<const float4*>(splat + id_nxt);
    r0 = p[0]; r1 = p[1]; r2 = p[2];
  }
};

// One round's records into LDS: lane j < n holds (in ga) the record of list position pos0 + j and tests it against the quarter's
// pixel rectangle as the colour kernels' gathering lanes do (only when the colour pass ran with its pre-cull, which is exact: a
// record it drops has no pixel with power >= threshold); the survivors are staged compacted, order preserved -- two 16-byte words
// {x, y, hA, nB} {hC, threshold, opacity, 0-based position in the tile's list} and the Gaussian's id; extra(slot) stores what
// else the pass stages beside a surviving record.  Returns the number staged (wave-uniform).  Opens with the barrier behind the
// previous round's LDS reads (single-wave workgroup) and closes with none: the caller requests the next round's records and the
// ids of the round after it where its own loads allow, and sets the barrier.
template <class Extra>
__device__ __forceinline__ int stage_cull(float4* s_rec, uint32_t* s_id, const Gather& ga, const QuarterGeom& g, int n,
                                          uint32_t pos0, int cull, Extra extra) {
  const int lane = threadIdx.x;
  const float wx0 = (float)g.qx0, wy0 = (float)g.qy0;
  __syncthreads();
  bool keep = false;
  float4 r1 = ga.r1;
  if (lane < n) {
    keep = cull ? (record_box_hits(ga.r0.x, ga.r0.y, ga.r2.z, ga.r2.w, wx0, wx0 + 7.0f, wy0, wy0 + 7.0f) &&
                   record_reaches_block(ga.r0.x, ga.r0.y, ga.r0.z, ga.r0.w, r1.x, r1.y, ga.r2.z, wx0, wx0 + 7.0f, wy0, wy0 + 7.0f))
                : true;
    r1.w = __uint_as_float(pos0 + (uint32_t)lane);
  }
  const uint64_t kept = __ballot(keep);
  if (keep) {
    const int slot = __popcll(kept & ((1ull << lane) - 1ull));
    s_id[slot] = ga.id_cur;
    extra(slot);
    s_rec[slot * 2 + 0] = ga.r0; s_rec[slot * 2 + 1] = r1;
  }
  return __popcll(kept);
}

// ---- a (pixel, record) pair ------------------------------------------------------------------------------------------------
// a, b: the staged words {x y hA nB} {hC thr opacity position}.  cull: the colour pass tested `power >= threshold` with the
// record's stored threshold (GGD_OPT_BLEND_CULL on) or with -inf (off).  A step hands its result to then(p) -- unless no pixel
// of the quarter gets past the wave-uniform skips, when it returns without (a continuation, not a flag in the result: the skip
// stays the plain branch to the next record that it is in the colour kernels).
__device__ __forceinline__ bool pair_need(const float4& a, const float4& b, const QuarterGeom& g, int cull, float& pw) {
  float dx, dy;
  pw = blend_power(a.x, a.y, a.z, a.w, b.x, (float)g.px, (float)g.py, dx, dy);
  const float thr = cull ? b.y : -__builtin_huge_valf();
  return __float_as_uint(b.w) < g.lastn && pw >= thr;
}

// forward, EXP_MODE the colour forward's (0, 1, 2; the default mode 3 runs the forward with the bare exponential, mode 1): the
// pixel blends the record (upd) with weight w = alpha Tr and goes on with transmittance test_T; w = 0 where it does not
struct PairForward { bool upd; float w, test_T; };
template <int EXP_MODE, class Then>
__device__ __forceinline__ void pair_forward(const float4& a, const float4& b, const QuarterGeom& g, int cull, float Tr,
                                             Then then) {
  float pw;
  const bool need = pair_need(a, b, g, cull, pw);
  if (__ballot(need) == 0ull) return;
  const float G = blend_exp<EXP_MODE>(pw);
  const float alpha = fminf(0.99f, G * b.z);
  const float test_T = Tr * (1.0f - alpha);
  const bool upd = need && !(pw > 0.0f) && !(alpha < ALPHA_FLOOR) && !(test_T < 0.0001f);
  then(PairForward{upd, upd ? alpha * Tr : 0.0f, test_T});
}

// ---- the round loops ---------------------------------------------------------------------------------------------------------
// ga: a Gather, or a type with its load_id / load_rec.  stage(n, pos0, pos_after_next) stages the round whose records ga holds --
// n entries from list position pos0 -- through stage_cull, requests the next loads with pos_after_next, the position of the round
// after the next one (any value for a round that does not exist: the loads are clamped), and returns the number of staged records.

// Front to back over the pixel's contributors; body(j, p) for every staged record j some pixel of the quarter needs, then the
// pixel's transmittance moves on.  Returns the transmittance behind the last contributor.
template <int EXP_MODE, class G, class Stage, class Body>
__device__ __forceinline__ float walk_front(const float4* s_rec, const QuarterGeom& g, int cull, G& ga, Stage stage, Body body) {
  float Tr = 1.0f;
  if (g.maxn > 0) { ga.load_id(0); ga.load_rec(); ga.load_id(ROUND); }
  for (uint32_t base = 0; base < g.maxn; base += ROUND) {
    const int ns = stage((int)min((uint32_t)ROUND, g.maxn - base), base, base + 2 * ROUND);
    for (int j = 0; j < ns; ++j) {
      pair_forward<EXP_MODE>(s_rec[j * 2 + 0], s_rec[j * 2 + 1], g, cull, Tr, [&](const PairForward& p) {
        body(j, p);
        Tr = p.upd ? p.test_T : Tr;
      });
    }
  }
  return Tr;
}

// ---- host: the prologue of a quarter pass's launch (4 T single-wave workgroups) -------------------------------------------------
// em: the exp mode of the colour pass of the same direction -- as ggd_launch_blend, the default mode 3 runs the forward with the
// bare exponential, mode 1; ggd_launch_blend_backward has an instance of its own for it
struct QuarterLaunch { int gx, T, em, cull; };
inline QuarterLaunch quarter_launch(const ggd_ctx* ctx, const ggd_params& prm, bool forward) {
  const int gx = (prm.width + 15) / 16, gy = (prm.height + 15) / 16;
  const int em = ctx->opt[GGD_OPT_EXP_MODE];
  return {gx, gx * gy, forward && em == 3 ? 1 : em, ctx->opt[GGD_OPT_BLEND_CULL] != 0};
}
