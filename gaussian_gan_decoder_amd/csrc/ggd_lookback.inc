// ggd_lookback.inc -- the two-level look-back over published status words that the depth sort (a onesweep pass over its tiles)
// and the row binning (level 1 of the folded form over its chunks) share, included inside the anonymous namespace of
// ggd_binning.hip and ggd_rowbin.hip.
// --------------------------------------------------------------------------------------------------- look-back --
// A status word = published flag (bit 30) | 30-bit count, written / read as single agent-scope relaxed atomics (the value IS
// the flag, so no fence is needed and the protocol is placement independent: per-XCD L2s are not coherent, agent-scope atomics
// bypass them).  Words are zero at launch; a workgroup only ever waits for lower-numbered ones, which are already running.
constexpr uint32_t STATUS_PUB = 1u << 30, STATUS_COUNT_MASK = STATUS_PUB - 1u;
constexpr int LOOKBACK_BATCH = 16;     // status words requested together while summing predecessors (batches are dependent round trips)

__device__ __forceinline__ uint32_t status_load(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void status_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum of `cnt` published words p[0], p[STRIDE], ...: LOOKBACK_BATCH requests in flight, unpublished ones are polled
template <int STRIDE>
__device__ __forceinline__ uint32_t lookback_sum(uint32_t* p, int cnt) {
  uint32_t acc = 0;
  for (int b0 = 0; b0 < cnt; b0 += LOOKBACK_BATCH) {
    uint32_t v[LOOKBACK_BATCH];
#pragma unroll
    for (int i = 0; i < LOOKBACK_BATCH; ++i) v[i] = (b0 + i < cnt) ? status_load(p + (size_t)(b0 + i) * STRIDE) : STATUS_PUB;
#pragma unroll
    for (int i = 0; i < LOOKBACK_BATCH; ++i) {
      uint32_t x = v[i];
      if ((x >> 30) == 0u) {
        uint32_t* q = p + (size_t)(b0 + i) * STRIDE;
        do { __builtin_amdgcn_s_sleep(1); x = status_load(q); } while ((x >> 30) == 0u);
      }
      acc += x & STATUS_COUNT_MASK;
    }
  }
  return acc;
}

// The sum over all EARLIER tiles of one column (a digit, a tile row) from a fixed two-level tree: tiles form groups of
// G = 2^gshift (G ~ sqrt(#tiles), ggd_group_shift); a tile publishes its count, sums the earlier tiles of its own group, the last
// tile of a group publishes the group aggregate, and every tile adds the aggregates of the earlier groups -- at most 2G
// independent loads, three dependent memory round trips.  (The classic decoupled look-back chain needs ~#tiles / 16 dependent
// round trips here: all tiles start together, so nobody finds an inclusive prefix nearby -- 15 round trips and 7.5 M uncached
// status loads per pass at 245 tiles, the 14 us floor the sort's passes used to have.)
// status: [rows tile words][group words], STRIDE words a row; col: the caller's column; gshift <= the shift the rows were laid
// out for (rs_status_words, ggd_fold_ctl_words).  TileT: the caller's index type (the shifts keep its signedness).  Returns
// start + the sum (start: where the caller's column begins, added first as the callers did).
template <int STRIDE, typename TileT>
__device__ __forceinline__ uint32_t lookback_two_level(uint32_t* status, int col, int rows, TileT tile, int gshift, uint32_t local,
                                                       uint32_t start) {
  const int grp = (int)(tile >> gshift), mem = (int)(tile & (((TileT)1 << gshift) - (TileT)1));
  uint32_t* tile_words = status + col;                             // [tile][STRIDE]
  uint32_t* group_words = status + (size_t)rows * STRIDE + col;    // [group][STRIDE]
  status_store(tile_words + (size_t)tile * STRIDE, STATUS_PUB | local);
  const uint32_t in_group = lookback_sum<STRIDE>(tile_words + ((size_t)grp << gshift) * STRIDE, mem);   // earlier tiles of my group
  if (mem == (1 << gshift) - 1) {   // the last tile of a group publishes the group's aggregate
    const uint32_t aggregate = STATUS_PUB | (in_group + local);
    status_store(group_words + (size_t)grp * STRIDE, aggregate);
  }
  return start + in_group + lookback_sum<STRIDE>(group_words, grp);                                             // earlier groups
}
