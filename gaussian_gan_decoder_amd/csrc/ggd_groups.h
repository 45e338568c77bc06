// ggd_groups.h -- the parameter groups of a fitted scene as ggd_densify.hip, ggd_mcmc.hip and ggd_adam.hip see them: six
// [P][width] float32 arrays in one order, each with its two Adam moments, and one launch over all of them in which every group
// owns a range of 256-thread workgroups.
#pragma once

#include "ggd_common.h"

enum { GG_XYZ, GG_F_DC, GG_F_REST, GG_OPACITY, GG_SCALING, GG_ROTATION, GG_GROUPS };   // the order of every pointer table (6 groups)
constexpr int GG_MAX_POINTS = 1 << 26;                                                 // rows of a model, for every entry point

struct ggd_row_group {
  const float* in[3];        // parameter, exp_avg, exp_avg_sq (moments NULL: this group has no optimizer state yet)
  float* out[3];             // (an in-place launch: the same arrays)
  uint32_t width;            // floats per row
  uint32_t first_block;      // this group's first workgroup of the launch
};

static inline int ggd_groups_check_M(ggd_ctx* ctx, const char* who, int32_t M) {
  return M < 1 || M > 16 ? ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": M (SH coefficients per channel) must be in [1, 16]") : GGD_OK;
}

// g[] of a launch over `rows` rows from the C ABI's two 18-pointer tables (M checked by the caller) and the launch's workgroups.
// A group of width 0 (f_rest at M = 1) has none: its first_block is the next group's.
static inline int ggd_groups_fill(ggd_ctx* ctx, const char* who, int32_t M, int32_t rows, const float* const* in18,
                                  float* const* out18, ggd_row_group (&g)[GG_GROUPS], uint64_t& blocks) {
  if (!in18 || !out18) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": NULL pointer table");
  const uint32_t widths[GG_GROUPS] = {3u, 3u, 3u * (uint32_t)(M - 1), 1u, 3u, 4u};
  blocks = 0;
  for (int k = 0; k < GG_GROUPS; ++k) {
    ggd_row_group& d = g[k];
    d.width = widths[k];
    d.first_block = (uint32_t)blocks;
    for (int j = 0; j < 3; ++j) { d.in[j] = in18[3 * k + j]; d.out[j] = out18[3 * k + j]; }
    if (d.width == 0) continue;
    if (!d.in[0] || !d.out[0]) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": NULL parameter pointer");
    const bool moments = d.out[1] != nullptr;
    if ((d.out[2] != nullptr) != moments || (moments && (!d.in[1] || !d.in[2])))
      return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": a group's moments are given together or not at all");
    blocks += ((uint64_t)rows * d.width + 255u) / 256u;
  }
  if (blocks > 0x7FFFFFFFull) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": too many elements for one launch");
  return GGD_OK;
}

// the scratch of an entry point: P in range, tmp usable, `need` bytes (the caller's layout at P; not read when P is refused)
static inline int ggd_check_tmp(ggd_ctx* ctx, const char* who, int32_t P, const void* tmp, size_t tmp_bytes, size_t need) {
  if (P < 0 || P > GG_MAX_POINTS) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": P must be in [0, 2^26]");
  if (!tmp || (reinterpret_cast<uintptr_t>(tmp) & 15u)) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": tmp is NULL or not 16-byte aligned");
  if (tmp_bytes < need) return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": tmp too small");
  return GGD_OK;
}

// The group of this workgroup: the last k with blockIdx.x >= g[k].first_block (a group without workgroups shares the next
// group's first_block or holds 0xFFFFFFFF, above every block index).
template <int N, class T>
__device__ __forceinline__ int ggd_block_group(const T (&g)[N]) {
  int G = 0;
#pragma unroll
  for (int k = 1; k < N; ++k)
    if (blockIdx.x >= g[k].first_block) G = k;
  return G;
}

// One thread per float of one group's rows: workgroup b of group G covers that group's elements [256 b, 256 b + 256).  The row
// is not checked against the launch's row count.
struct ggd_group_elem { int G; uint32_t row, col; };
__device__ __forceinline__ ggd_group_elem ggd_group_walk(const ggd_row_group (&g)[GG_GROUPS]) {
  const int G = ggd_block_group(g);
  const ggd_row_group& grp = g[G];
  const uint32_t w = grp.width;
  const uint64_t e0 = (uint64_t)(blockIdx.x - grp.first_block) * 256u;
  const uint32_t row0 = (uint32_t)(e0 / w);                                  // (uniform)
  const uint32_t off = (uint32_t)(e0 - (uint64_t)row0 * w) + threadIdx.x;    // < w + 256
  const uint32_t dr = off / w;
  return {G, row0 + dr, off - dr * w};
}
