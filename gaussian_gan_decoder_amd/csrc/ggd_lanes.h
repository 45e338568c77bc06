// ggd_lanes.h -- cross-lane primitives of a 64-lane wave that stay in the vector registers (gfx950): DPP row moves, the lane-block
// swaps v_permlane16_swap / v_permlane32_swap and v_readlane, where __shfl / __shfl_up / __shfl_xor each cost a trip through the
// LDS pipe (ds_bpermute_b32 + s_waitcnt lgkmcnt(0)).  Builtins, not inline asm: the compiler's hazard recogniser pads the DPP and
// permlane reads itself.
//
// RULE for every function here: ALL 64 LANES OF THE WAVE MUST BE ACTIVE AT THE CALL (wave-uniform control flow: `if (wv == 0)`,
// `if (tid < 64)`, a loop whose bound is the same in every lane).  A DPP or permlane read of an inactive lane returns that lane's
// stale register, not a defined value, and v_readlane needs a lane index that is the same in every lane.  As with the shuffles they
// replace, a call never stands inside a select (`c ? lane_xor<8>(x) : y` may be sunk into a branch by the compiler).
//
// 32-bit integers (uint32_t, int): that is all the front-end kernels move.  The scan and wave_sum_lane63 also take float (the camera
// backward's sums): the additions then happen in the scan's fixed tree, so the result is the same from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace ggd_lanes_detail {
// DPP controls (the dpp_ctrl field of the VOP DPP encoding)
constexpr int DPP_QUAD_XOR1 = 0xB1;      // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;      // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_SHR = 0x110;       // + n: row_shr:n (lane i of a 16-lane row reads lane i - n; none below the row's start)
constexpr int DPP_ROW_ROR = 0x120;       // + n: row_ror:n (lane i reads lane (i - n) mod 16 of its row)
constexpr int DPP_ROW_BCAST15 = 0x142;   // lane 15 of every row to all lanes of the next row
constexpr int DPP_ROW_BCAST31 = 0x143;   // lane 31 to all lanes of rows 2 and 3

// `v` moved by CTRL; lanes that the move does not write (outside ROW_MASK / BANK_MASK, or without a source lane) get `old`
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, typename T>
__device__ __forceinline__ T dpp(T old, T v) {
  static_assert(sizeof(T) == 4 && (std::is_integral<T>::value || std::is_same<T, float>::value), "32-bit integers or float");
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK,
                                                           BANK_MASK, false));
}

struct op_add { template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a + b; } };
struct op_max { template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a > b ? a : b; } };

// Inclusive scan of `v` over the 64 lanes under an associative, commutative Op with identity `id`: four steps inside the 16-lane
// rows (row_shr 1, 2, 4, 8), row 0 -> 1 and 2 -> 3 (row_bcast:15 into rows 1 and 3), rows 0-1 -> 2-3 (row_bcast:31).  Every step is
// one VALU instruction (the move folds into the add / max as its DPP operand).
template <typename Op, typename T>
__device__ __forceinline__ T scan(T v, T id) {
  v = Op::f(v, dpp<DPP_ROW_SHR + 1>(id, v));
  v = Op::f(v, dpp<DPP_ROW_SHR + 2>(id, v));
  v = Op::f(v, dpp<DPP_ROW_SHR + 4>(id, v));
  v = Op::f(v, dpp<DPP_ROW_SHR + 8>(id, v));
  v = Op::f(v, dpp<DPP_ROW_BCAST15, 0xa>(id, v));
  v = Op::f(v, dpp<DPP_ROW_BCAST31, 0xc>(id, v));
  return v;
}
}  // namespace ggd_lanes_detail

// x of lane `uniform_lane`, in every lane (a scalar: v_readlane_b32).  uniform_lane must hold the same value, 0 .. 63, in all lanes;
// it need not be known to the compiler as uniform (it is taken from the first lane).  All 64 lanes active.
template <typename T>
__device__ __forceinline__ T wave_pick(T x, int uniform_lane) {
  static_assert(sizeof(T) == 4 && std::is_integral<T>::value, "32-bit integers");
  return (T)__builtin_amdgcn_readlane((int)x, __builtin_amdgcn_readfirstlane(uniform_lane));
}

// Inclusive prefix sum over the lanes (wraps like the type).  All 64 lanes active.
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
  return ggd_lanes_detail::scan<ggd_lanes_detail::op_add>(v, (T)0);
}

// Sum / maximum of v over the wave; the `_lane63` forms leave it in lane 63 only (other lanes: the prefix up to them), for a single
// writer; the `_to_all` forms return it in every lane (as a scalar).  All 64 lanes active.
template <typename T>
__device__ __forceinline__ T wave_sum_lane63(T v) { return wave_inclusive_scan(v); }
template <typename T>
__device__ __forceinline__ T wave_max_lane63(T v) {
  return ggd_lanes_detail::scan<ggd_lanes_detail::op_max>(v, v);   // (a lane without a source keeps its own value)
}
template <typename T>
__device__ __forceinline__ T wave_sum_to_all(T v) { return wave_pick(wave_sum_lane63(v), 63); }
template <typename T>
__device__ __forceinline__ T wave_max_to_all(T v) { return wave_pick(wave_max_lane63(v), 63); }

// x of lane (lane ^ D), D = 1, 2, 4, 8, 16, 32.  All 64 lanes active.
//   1, 2   one DPP move (quad_perm)
//   8      one DPP move (row_ror:8)
//   4      two DPP moves: row_ror:12 into the banks whose lanes have bit 2 clear, row_ror:4 into the others
//   16, 32 one lane-block swap of x with a copy of itself, and a select between the two results
template <int D, typename T>
__device__ __forceinline__ T lane_xor(T x) {
  using namespace ggd_lanes_detail;
  static_assert(sizeof(T) == 4 && std::is_integral<T>::value, "32-bit integers");
  static_assert(D == 1 || D == 2 || D == 4 || D == 8 || D == 16 || D == 32, "lane distance");
  if constexpr (D == 1) return dpp<DPP_QUAD_XOR1>(x, x);
  else if constexpr (D == 2) return dpp<DPP_QUAD_XOR2>(x, x);
  else if constexpr (D == 4) return dpp<DPP_ROW_ROR + 4, 0xf, 0xa>(dpp<DPP_ROW_ROR + 12, 0xf, 0x5>(x, x), x);
  else if constexpr (D == 8) return dpp<DPP_ROW_ROR + 8>(x, x);
  else {
    // after the swap r[0] holds the even blocks' x in both blocks of a pair, r[1] the odd blocks'
    const auto r = D == 16 ? __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false)
                           : __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    return (T)((threadIdx.x & (unsigned)D) ? r[0] : r[1]);
  }
}

// x + x of lane (lane ^ D), in both lanes of the pair.  For D = 16, 32 the two results of the lane-block swap are the pair's two
// values in every lane: their sum needs no select.  All 64 lanes active.
template <int D, typename T>
__device__ __forceinline__ T lane_pair_sum(T x) {
  static_assert(sizeof(T) == 4 && std::is_integral<T>::value, "32-bit integers");
  if constexpr (D == 16 || D == 32) {
    const auto r = D == 16 ? __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false)
                           : __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    return (T)(r[0] + r[1]);
  } else {
    return x + lane_xor<D>(x);
  }
}

// 64 x 64 bit-matrix transpose across the wave: lane i passes row i (bit b = M[i][b]) and gets column `lane` (bit i = M[i][lane]).
// Six butterfly stages (block sizes 32 .. 1): in every lane pair (l, l ^ d) the off-diagonal d x d blocks are exchanged.
//   32     v_permlane32_swap(lo, hi): the upper half-wave's low words against the lower half-wave's high words -- the exchange itself
//   16     per word one v_permlane16_swap with a copy: every lane then holds the word of both partners, one v_perm_b32 (byte
//          selector by lane) puts the two halves together
//   8      row_ror:8 brings the partner's word, one v_perm_b32
//   4 .. 1 DPP moves bring the partner's word; rotate (by d, or 32 - d in the lower partner) and bit-select with the lane's mask
// All 64 lanes active.
__device__ __forceinline__ uint64_t wave_transpose64(uint64_t row) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t w[2] = {(uint32_t)row, (uint32_t)(row >> 32)};
  {
    const auto r = __builtin_amdgcn_permlane32_swap(w[0], w[1], false, false);
    w[0] = r[0]; w[1] = r[1];
  }
  // v_perm_b32(S0, S1, sel): selector bytes 0-3 take bytes of S1, 4-7 of S0
  const uint32_t sel16 = (lane & 16u) ? 0x07060302u : 0x05040100u;   // upper partner: both high halves; lower: both low halves
  const uint32_t sel8 = (lane & 8u) ? 0x03070105u : 0x06020400u;     // {own, partner} = {S1, S0}
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const auto r = __builtin_amdgcn_permlane16_swap(w[k], w[k], false, false);   // r[0]: the lower partner's word, r[1]: the upper's
    w[k] = __builtin_amdgcn_perm(r[1], r[0], sel16);
    w[k] = __builtin_amdgcn_perm(lane_xor<8>(w[k]), w[k], sel8);
  }
  auto stage = [&](auto dist, uint32_t M) {
    constexpr int D = decltype(dist)::value;
    const bool up = (lane & (uint32_t)D) != 0;
    const uint32_t keep = up ? ~M : M, rot = up ? (uint32_t)D : 32u - (uint32_t)D;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t p = lane_xor<D>(w[k]);
      w[k] = (w[k] & keep) | (__builtin_amdgcn_alignbit(p, p, rot) & ~keep);   // (the bits a rotation wraps around fall outside ~keep)
    }
  };
  stage(std::integral_constant<int, 4>(), 0x0F0F0F0Fu);
  stage(std::integral_constant<int, 2>(), 0x33333333u);
  stage(std::integral_constant<int, 1>(), 0x55555555u);
  return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
}
