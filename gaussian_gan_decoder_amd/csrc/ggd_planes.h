// ggd_planes.h -- what every kernel sampling the feature planes shares (ggd_triplane.hip: the gather / scatter kernels;
// ggd_density.hip: the fused density field): the plane set as the host functions pass it on, the plane axes, and the tap
// arithmetic of grid_sample (bilinear / trilinear, zero padding, align_corners = False) -- the cell of a sample on one plane
// and the weight, the inside test and the texel of its tap k.
#pragma once

#include "ggd_common.h"

// One set of three feature planes, channel-last: [3][H][W][C] (D = 0, the 2-D tri-plane form) or [3][D][H][W][C] (tri-grid).
// axes: 0 = EG3D plane axes, 1 = PanoHead (grid_uvw below); positions are scaled by 2 / box_warp onto [-1, 1].
struct ggd_plane_set {
  const float* grids_cl = nullptr;   // NULL where only the geometry is used (the scatter writes a gradient buffer of this shape)
  int C = 0, D = 0, H = 0, W = 0, axes = 0;
  float box_warp = 1.0f;
};

// the axes and depth a plane set may have; the one refusal that every caller of the samplers shares (`who` names the caller)
static inline bool ggd_plane_axes_ok(const ggd_plane_set& ps) {
  return ps.axes >= 0 && ps.axes <= 1 && ps.D >= 0 && (ps.D > 0 || ps.axes == 0);
}
static inline int ggd_check_plane_set(ggd_ctx* ctx, const char* who, const ggd_plane_set& ps) {
  if (ggd_plane_axes_ok(ps)) return GGD_OK;
  return ggd_fail(ctx, GGD_E_INVALID, std::string(who) + ": bad axes / depth (the 2-D form has the EG3D axes only)");
}

#ifdef __HIPCC__
// Is the tap at floor(i) + o (o = 0 / 1) inside [0, size)?  Tested on the FLOAT floor: for a coordinate beyond the int range
// (+-1e30, +-inf) (int)floorf() saturates and x0 + 1 overflows, which the compiler may treat -- and for `x1 >= 0 && x1 < W`
// did treat -- as inside.  The same decision as the integer test for every coordinate that fits an int; false for NaN.
// Where this is false for such a coordinate the integers x0, x0 + 1 .. of the cell (below) are MEANINGLESS (the conversion and
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

// The cell of a sample on plane p: its pixel coordinates and their float floors (what tap_inside tests); the fractions are
// formed where they are used.  It holds no integers: those come from cell_corner / tap_at below and are sound only under the
// test (see tap_inside).  G3 = false: the 2-D form, iz = fz = 0.
struct PlaneCell {
  float ix, iy, iz, fx, fy, fz;
  __device__ __forceinline__ float ax() const { return ix - fx; }
  __device__ __forceinline__ float ay() const { return iy - fy; }
  __device__ __forceinline__ float az() const { return iz - fz; }
};

template <bool G3>
static __device__ __forceinline__ PlaneCell plane_cell(int axes, int p, float x, float y, float z, int D, int H, int W) {
  float u, v, w = 0.0f;
  if (G3) grid_uvw(axes, p, x, y, z, u, v, w); else plane_uv(p, x, y, z, u, v);
  // grid_sample, align_corners = False: pixel = ((g + 1) * size - 1) / 2
  const float ix = ((u + 1.0f) * (float)W - 1.0f) * 0.5f;
  const float iy = ((v + 1.0f) * (float)H - 1.0f) * 0.5f;
  const float iz = G3 ? ((w + 1.0f) * (float)D - 1.0f) * 0.5f : 0.0f;
  return PlaneCell{ix, iy, iz, floorf(ix), floorf(iy), floorf(iz)};
}

// Tap k of a cell (k = 0 .. 3, 0 .. 7 with G3): bit 0 steps in x, bit 1 in y, bit 2 in z.
// its weight, in grid_sampler's order: (x) * (y) [* (z)]
template <bool G3>
static __device__ __forceinline__ float tap_weight(const PlaneCell& c, int k) {
  const float ax = c.ax(), ay = c.ay();
  float wk = ((k & 1) ? ax : 1.0f - ax) * ((k & 2) ? ay : 1.0f - ay);
  if (G3) { const float az = c.az(); wk = wk * ((k & 4) ? az : 1.0f - az); }
  return wk;
}
// is it inside the grid? (D: the grid's depth, unused without G3)
template <bool G3>
static __device__ __forceinline__ bool tap_in(const PlaneCell& c, int k, int D, int H, int W) {
  return tap_inside(c.fx, k & 1, W) && tap_inside(c.fy, (k >> 1) & 1, H) && (!G3 || tap_inside(c.fz, k >> 2, D));
}
// The integer coordinates of the cell's corner (tap 0) and of tap k (z: the depth slice, the row of a [D][C] modulation
// table; 0 without G3), to be used only under tap_in(c, k) or another range test of the floors (see tap_inside), and the
// tap's texel within its plane, in texels.
struct PlaneTap { int x, y, z; };
template <bool G3>
static __device__ __forceinline__ PlaneTap cell_corner(const PlaneCell& c) { return PlaneTap{(int)c.fx, (int)c.fy, G3 ? (int)c.fz : 0}; }
template <bool G3>
static __device__ __forceinline__ PlaneTap tap_at(const PlaneTap& corner, int k) {
  return PlaneTap{corner.x + (k & 1), corner.y + ((k >> 1) & 1), G3 ? corner.z + (k >> 2) : 0};
}
static __device__ __forceinline__ size_t tap_texel(const PlaneTap& t, int H, int W) { return ((size_t)t.z * H + t.y) * W + t.x; }
#endif
