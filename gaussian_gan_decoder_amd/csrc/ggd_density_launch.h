// ggd_density_launch.h -- the density field for other translation units (ggd_teacher.hip): its weights as a bundle, its
// refusals, and density_kernel over pos[N][3] as ggd_density_points launches it.  Defined in ggd_density.hip.
#pragma once
#include "ggd_common.h"
#include "ggd_planes.h"

// OSGDecoder's weights: w1 [64][32], b1 [64], w2 [33][64], b2 [33] (row 0: sigma); act: the rgb activation (dn_act)
struct ggd_field_weights {
  const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
  int act = 0;
};

// The field's refusals that need no point: channel count, axes / depth, activation.  `who` names the caller in the error text.
int ggd_check_field(ggd_ctx* ctx, const char* who, const ggd_plane_set& ps, const ggd_field_weights& fw);

// Checks its arguments like the C entry (ggd_check_field first; N <= 0 launches nothing).  rgb may be NULL.
int ggd_launch_density_points(ggd_ctx* ctx, hipStream_t s, const char* who, const ggd_plane_set& ps, const ggd_field_weights& fw,
                              const float* pos, int64_t N, float* sigma, float* rgb);
