// ggd_mlp_gelu.inc -- GELU / GELU' from LDS interpolation tables (included inside ggd_mlp.hip's anonymous namespace).
//
// Evaluated from exponentials and polynomials at fp32 accuracy these cost 21 / 22 issue slots per value -- 1.5 ms of the
// forward, 1.5 ms of the backward and 1.2 ms of the weight-gradient kernel per 2 M-point step were nothing else.  Both are
// smooth, bounded, saturating functions of ONE variable: Phi(x) (gelu = x Phi) and gelu'(x) = Phi(x) + x phi(x) are tabulated
// on [-6, 6] (beyond, both are 0 / 1 to 1e-9; the index clamps) as linear pieces {f(x_i), f(x_i+1) - f(x_i)}, fine enough for
// the consumer: 2048 intervals for the forward's Phi (error 1.1e-6; 16 KB), 4095 for the backward's gelu' (8e-7; 32 KB: what
// is left of the CU's 160 KB beside the two weight buffers), 1024 for the weight gradients' Phi, whose a = gelu(z) is rounded to
// fp16 next (4e-6; 8 KB: two workgroups per CU still fit).  Per value: fma, clamp, floor, subtract, convert, one 8-byte LDS read,
// one FMA.  (Interpolating QUADRATICS on 1024 intervals, 16 bytes per entry, were tried first: the compiler hoisted the 16-byte
// reads of a whole tile group and spilled 470 - 720 VGPRs; 23.5 / 19.7 ms for the forward / backward.)  Built once per context
// in double precision (hl_tables_kernel).
constexpr int GT_N_FWD = 2048, GT_N_BWD = 4095, GT_N_WG = 1024;
constexpr int gt_bytes(int n) { return ((n + 1) * 8 + 15) & ~15; }
constexpr int GT_OFF_FWD = 0, GT_OFF_BWD = gt_bytes(GT_N_FWD), GT_OFF_WG = GT_OFF_BWD + gt_bytes(GT_N_BWD);
constexpr int GT_BYTES = GT_OFF_WG + gt_bytes(GT_N_WG);
template <int N>
__device__ __forceinline__ float gt_lin(const float2* __restrict__ tbl, float x) {
  float t = __builtin_fmaf(x, (float)N / 12.0f, 0.5f * (float)N);      // (x + 6) * N / 12
  t = __builtin_amdgcn_fmed3f(t, 0.0f, (float)N - 0.001f);             // NaN -> 0
  const float fl = __builtin_floorf(t);
  const float2 c = tbl[(int)fl];
  return __builtin_fmaf(c.y, t - fl, c.x);
}
// Four look-ups as ONE instruction block (forward / backward kernels): through the compiler the LDS reads of a whole tile
// group were hoisted together and -- these kernels sit at their 256-register limit -- 260 - 450 VGPRs were spilled (forward
// 23.5 ms).  Here the block's 16 temporaries live for its 30 instructions and are dead outside.  x -> f(x) in place.
// tbl: LDS byte address of the table (wave-uniform); sc, hf, hi: N / 12, N / 2, N - 0.001 held in VGPRs by the caller.
__device__ __forceinline__ void gt_lin4(uint32_t tbl, float sc, float hf, float hi, float& x0, float& x1, float& x2, float& x3) {
  // (round 5: one ds_read_b64 per value instead of two ds_read_b32 -- the {f, df} pair is one aligned 8-byte word; per-lane
  // addresses over a 16 - 32 KB table collide in the 32 banks either way, but half the LDS instructions halve the conflict
  // cycles: 58 - 63 % of the LDS pipe's active cycles in these kernels were bank conflicts, profiles/r04/pmc_summary_decoder_fp32.txt.
  // The four 64-bit destinations are FIXED registers v[248:255] (clobbered): inline asm cannot name the halves of a 64-bit
  // operand, and with the FMAs outside the block the kernels -- at their 256-register limit -- spilled: 4.8 -> 10.8 ms)
  float f0, f1, f2, f3;
  uint32_t a0, a1, a2, a3;
  asm volatile(
      "v_fma_f32 %0, %0, %12, %13\n\tv_fma_f32 %1, %1, %12, %13\n\tv_fma_f32 %2, %2, %12, %13\n\tv_fma_f32 %3, %3, %12, %13\n\t"
      "v_med3_f32 %0, %0, 0, %14\n\tv_med3_f32 %1, %1, 0, %14\n\tv_med3_f32 %2, %2, 0, %14\n\tv_med3_f32 %3, %3, 0, %14\n\t"
      "v_cvt_u32_f32 %8, %0\n\tv_cvt_u32_f32 %9, %1\n\tv_cvt_u32_f32 %10, %2\n\tv_cvt_u32_f32 %11, %3\n\t"
      "v_lshl_add_u32 %8, %8, 3, %15\n\tv_lshl_add_u32 %9, %9, 3, %15\n\tv_lshl_add_u32 %10, %10, 3, %15\n\tv_lshl_add_u32 %11, %11, 3, %15\n\t"
      "ds_read_b64 v[248:249], %8\n\tds_read_b64 v[250:251], %9\n\tds_read_b64 v[252:253], %10\n\tds_read_b64 v[254:255], %11\n\t"
      "v_fract_f32 %4, %0\n\tv_fract_f32 %5, %1\n\tv_fract_f32 %6, %2\n\tv_fract_f32 %7, %3\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_fma_f32 %0, v249, %4, v248\n\tv_fma_f32 %1, v251, %5, v250\n\tv_fma_f32 %2, v253, %6, v252\n\tv_fma_f32 %3, v255, %7, v254"
      : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "=&v"(f0), "=&v"(f1), "=&v"(f2), "=&v"(f3), "=&v"(a0), "=&v"(a1), "=&v"(a2),
        "=&v"(a3)
      : "v"(sc), "v"(hf), "v"(hi), "s"(tbl)
      : "memory", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255");
}
__global__ __launch_bounds__(256) void hl_tables_kernel(unsigned char* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  auto Phi = [](double x) { return 0.5 * erfc(-x * 0.70710678118654752440); };
  auto dG = [&](double x) { return Phi(x) + x * exp(-0.5 * x * x) * 0.39894228040143267794; };
  auto fill = [&](float2* tbl, int n, bool grad) {
    if (i > n) return;
    const double h = 12.0 / n, x0 = -6.0 + i * h, x1 = i < n ? x0 + h : x0;
    const double f0 = grad ? dG(x0) : Phi(x0), f1 = grad ? dG(x1) : Phi(x1);
    tbl[i] = make_float2((float)f0, (float)(f1 - f0));
  };
  fill(reinterpret_cast<float2*>(out + GT_OFF_FWD), GT_N_FWD, false);
  fill(reinterpret_cast<float2*>(out + GT_OFF_BWD), GT_N_BWD, true);
  fill(reinterpret_cast<float2*>(out + GT_OFF_WG), GT_N_WG, false);
}
// every thread of the workgroup copies its share of `bytes` (a multiple of 16) of a table into LDS
__device__ __forceinline__ void gt_load(unsigned char* lds, const unsigned char* __restrict__ src, int bytes, int tid, int nthreads) {
  for (int k = tid; k < bytes / 16; k += nthreads) reinterpret_cast<uint4*>(lds)[k] = reinterpret_cast<const uint4*>(src)[k];
}

