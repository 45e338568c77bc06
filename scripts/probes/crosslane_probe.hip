// Probe: latency of a chain of DEPENDENT cross-lane steps, through the LDS pipe (__shfl*: ds_bpermute_b32 + s_waitcnt) against the
// register forms of csrc/ggd_lanes.h (DPP, v_permlane*_swap, v_readlane), at 1 and at 4 waves per SIMD.
//   scan       the six-step 64-lane inclusive scan
//   transpose  one 64 x 64 bit-matrix transpose (six butterfly stages on two words)
//   pick       x of a wave-uniform lane the compiler cannot prove uniform
//   xor4       lane ^ 4: __shfl_xor, two DPP moves (bank masks), ds_swizzle
// Every kernel runs REPS chains, each fed by the one before; time per chain from wall_clock64 (100 MHz) brackets of every wave's
// loop (median over the waves) and from events around the launch.
// Build + run on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Igaussian_gan_decoder_amd/csrc scripts/probes/crosslane_probe.hip -o crosslane_probe && ./crosslane_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ggd_lanes.h"
#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); exit(1); } } while (0)

namespace shfl {   // the forms the kernels had
__device__ __forceinline__ uint32_t scan(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
template <int D, uint32_t M>
__device__ __forceinline__ void tr_stage(uint32_t& lo, uint32_t& hi, uint32_t lane) {
  const bool up = (lane & (uint32_t)D) != 0;
  const uint32_t keep = up ? ~M : M;
  const uint32_t slo = up ? ((lo & M) << D) : ((lo & ~M) >> D);
  const uint32_t shi = up ? ((hi & M) << D) : ((hi & ~M) >> D);
  lo = (lo & keep) | (uint32_t)__shfl_xor((int)slo, D, 64);
  hi = (hi & keep) | (uint32_t)__shfl_xor((int)shi, D, 64);
}
__device__ __forceinline__ uint64_t transpose64(uint64_t row) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t lo = (uint32_t)row, hi = (uint32_t)(row >> 32);
  {
    const bool up = (lane & 32u) != 0;
    const uint32_t recv = (uint32_t)__shfl_xor((int)(up ? lo : hi), 32, 64);
    if (up) lo = recv; else hi = recv;
  }
  tr_stage<16, 0x0000FFFFu>(lo, hi, lane);
  tr_stage<8, 0x00FF00FFu>(lo, hi, lane);
  tr_stage<4, 0x0F0F0F0Fu>(lo, hi, lane);
  tr_stage<2, 0x33333333u>(lo, hi, lane);
  tr_stage<1, 0x55555555u>(lo, hi, lane);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
}  // namespace shfl

enum { SCAN_SHFL, SCAN_DPP, TR_SHFL, TR_NEW, PICK_SHFL, PICK_READLANE, XOR4_SHFL, XOR4_DPP, XOR4_SWIZZLE, N_KINDS };
constexpr int REPS = 1000;

template <int KIND>
__global__ __launch_bounds__(1024) void probe(uint32_t* out, long long* ticks, uint32_t seed) {
  const int wv = threadIdx.x >> 6;
  uint32_t x = seed * 2654435761u + threadIdx.x * 40503u + blockIdx.x;
  uint64_t r = ((uint64_t)x << 32) | (x * 2246822519u);
  const long long t0 = wall_clock64();
#pragma unroll 4
  for (int i = 0; i < REPS; ++i) {
    if constexpr (KIND == SCAN_SHFL) x = shfl::scan(x) ^ (uint32_t)i;
    else if constexpr (KIND == SCAN_DPP) x = wave_inclusive_scan(x) ^ (uint32_t)i;
    else if constexpr (KIND == TR_SHFL) r = shfl::transpose64(r) + (uint64_t)i;
    else if constexpr (KIND == TR_NEW) r = wave_transpose64(r) + (uint64_t)i;
    else if constexpr (KIND == PICK_SHFL) x = (uint32_t)__shfl((int)x, (wv * 5 + i) & 63, 64) + threadIdx.x;
    else if constexpr (KIND == PICK_READLANE) x = wave_pick(x, (wv * 5 + i) & 63) + threadIdx.x;
    else if constexpr (KIND == XOR4_SHFL) x = (uint32_t)__shfl_xor((int)x, 4, 64) + (uint32_t)i;
    else if constexpr (KIND == XOR4_DPP) x = lane_xor<4>(x) + (uint32_t)i;
    else if constexpr (KIND == XOR4_SWIZZLE) x = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x101F) + (uint32_t)i;   // xor_mask 4
  }
  const long long t1 = wall_clock64();
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = x ^ (uint32_t)r ^ (uint32_t)(r >> 32);
  if ((threadIdx.x & 63) == 0) ticks[(size_t)blockIdx.x * (blockDim.x >> 6) + wv] = t1 - t0;
}

template <int KIND>
static void run(const char* name, int wavesPerSimd, std::vector<uint32_t>* result) {
  const int CUS = 256, threads = 256 * wavesPerSimd, waves = CUS * threads / 64;   // one workgroup per CU, 4 SIMDs per CU
  uint32_t* out; long long* ticks;
  CK(hipMalloc(&out, (size_t)CUS * threads * 4)); CK(hipMalloc(&ticks, (size_t)waves * 8));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  probe<KIND><<<CUS, threads>>>(out, ticks, 1u);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  probe<KIND><<<CUS, threads>>>(out, ticks, 1u);
  CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms; CK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<long long> t(waves); CK(hipMemcpy(t.data(), ticks, (size_t)waves * 8, hipMemcpyDeviceToHost));
  std::sort(t.begin(), t.end());
  const double ns_med = t[waves / 2] * 10.0 / REPS, ns_min = t[0] * 10.0 / REPS, ns_max = t[waves - 1] * 10.0 / REPS;
  printf("%-34s waves/SIMD=%d  per chain: %7.1f ns median (%.1f .. %.1f) = %6.1f cycles @2.4GHz; launch %.3f ms = %.1f ns per chain\n",
         name, wavesPerSimd, ns_med, ns_min, ns_max, ns_med * 2.4, ms, ms * 1e6 / REPS);
  if (result) { result->resize((size_t)CUS * threads); CK(hipMemcpy(result->data(), out, result->size() * 4, hipMemcpyDeviceToHost)); }
  CK(hipFree(out)); CK(hipFree(ticks));
}

int main() {
  int bad = 0;
  for (int w : {1, 4}) {
    std::vector<uint32_t> a, b;
    run<SCAN_SHFL>("scan: 6 x __shfl_up", w, &a); run<SCAN_DPP>("scan: 6 x DPP add", w, &b);
    if (a != b) { printf("MISMATCH scan\n"); ++bad; }
    run<TR_SHFL>("transpose: 11 x __shfl_xor", w, &a); run<TR_NEW>("transpose: swaps + DPP", w, &b);
    if (a != b) { printf("MISMATCH transpose\n"); ++bad; }
    run<PICK_SHFL>("pick: __shfl(x, uniform)", w, &a); run<PICK_READLANE>("pick: v_readlane", w, &b);
    if (a != b) { printf("MISMATCH pick\n"); ++bad; }
    run<XOR4_SHFL>("lane ^ 4: __shfl_xor", w, &a); run<XOR4_DPP>("lane ^ 4: 2 x DPP row_ror", w, &b);
    if (a != b) { printf("MISMATCH xor4 dpp\n"); ++bad; }
    run<XOR4_SWIZZLE>("lane ^ 4: ds_swizzle", w, &b);
    if (a != b) { printf("MISMATCH xor4 swizzle\n"); ++bad; }
  }
  return bad ? 1 : 0;
}
