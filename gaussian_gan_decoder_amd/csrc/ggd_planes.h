// ggd_planes.h -- the pieces of the plane gather that every kernel sampling the feature planes shares (ggd_triplane.hip: the
// gather / scatter kernels; ggd_density.hip: the fused density field): the inside test of a tap and the plane axes.
#pragma once

#include <hip/hip_runtime.h>

#ifdef __HIPCC__
// Is the tap at floor(i) + o (o = 0 / 1) inside [0, size)?  Tested on the FLOAT floor: for a coordinate beyond the int range
// (+-1e30, +-inf) (int)floorf() saturates and x0 + 1 overflows, which the compiler may treat -- and for `x1 >= 0 && x1 < W`
// did treat -- as inside.  The same decision as the integer test for every coordinate that fits an int; false for NaN.
// Where this is false for such a coordinate the integers x0, x0 + 1 .. the callers derive are MEANINGLESS (the conversion and
// the increment are undefined there, not merely saturated): use them only under this test, never in a range test of their own.
static __device__ __forceinline__ bool tap_inside(float f, int o, int size) {
  const float t = f + (float)o;
  return t >= 0.0f && t <= (float)(size - 1);
}

// EG3D plane axes of the 2-D tri-plane form: plane 0 -> (x, y), plane 1 -> (x, z), plane 2 -> (z, x)
static __device__ __forceinline__ void plane_uv(int p, float x, float y, float z, float& u, float& v) {
  if (p == 0) { u = x; v = y; } else if (p == 1) { u = x; v = z; } else { u = z; v = x; }
}

// Tri-grid: (u, v, w) index (W, H, D).  axes: 0 = EG3D plane axes (plane 2 -> (z, x, y)), 1 = PanoHead (plane 2 -> (y, z, x));
// plane 0 -> (x, y, z), plane 1 -> (x, z, y) in both.
static __device__ __forceinline__ void grid_uvw(int axes, int p, float x, float y, float z, float& u, float& v, float& w) {
  if (p == 0) { u = x; v = y; w = z; }
  else if (p == 1) { u = x; v = z; w = y; }
  else if (axes == 0) { u = z; v = x; w = y; }
  else { u = y; v = z; w = x; }
}
#endif
