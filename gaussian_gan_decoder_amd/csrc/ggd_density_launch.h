// ggd_density_launch.h -- the density field's launch for other translation units (ggd_teacher.hip): density_kernel over
// pos[N][3], as ggd_density_points launches it.  Defined in ggd_density.hip.  Checks its arguments like the C entry (with
// N = 0 it checks C / axes / D / act and launches nothing); `who` names the caller in the error text.
#pragma once
#include "ggd_common.h"

int ggd_launch_density_points(ggd_ctx* ctx, hipStream_t s, const char* who, const float* grids_cl, int C, int D, int H, int W,
                              int axes, float box_warp, const float* w1, const float* b1, const float* w2, const float* b2, int act,
                              const float* pos, int64_t N, float* sigma, float* rgb);
