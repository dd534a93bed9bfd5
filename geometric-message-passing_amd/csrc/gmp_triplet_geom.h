// The per-triplet and per-edge arithmetic of K11's geometry, shared by the node-form kernels
// (gmp_triplet.hip: u, v from pos) and the vector-form kernels (gmp_triplet_pbc.hip: u, v from
// the per-edge vectors of a periodic graph).  The fp32 helpers reproduce the reference's torch
// CPU evaluation operation by operation (see gmp_triplet.hip).
#pragma once
#include "gmp_common.h"

namespace gmp {
namespace {

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 ld3(const float* __restrict__ p, int64_t a) {
  return V3{p[3 * a], p[3 * a + 1], p[3 * a + 2]};
}
__device__ __forceinline__ V3 sub3(V3 a, V3 b) {
  return V3{__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z)};
}
__device__ __forceinline__ V3 add3(V3 a, V3 b) {
  return V3{__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z)};
}
// torch.cross on CPU: fma(a_i, b_j, -(a_j * b_i))
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
  return V3{__fmaf_rn(a.y, b.z, -__fmul_rn(a.z, b.y)), __fmaf_rn(a.z, b.x, -__fmul_rn(a.x, b.z)),
            __fmaf_rn(a.x, b.y, -__fmul_rn(a.y, b.x))};
}
// (a * b).sum(-1): the reduction starts from +0, so an all-(-0) sum is +0 (atan2(0, +0) = 0,
// not pi, for a degenerate self-loop vector)
__device__ __forceinline__ float dot3(V3 a, V3 b) {
  return __fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(a.x, b.x)), __fmul_rn(a.y, b.y)),
                   __fmul_rn(a.z, b.z));
}
// a.norm(dim=-1)
__device__ __forceinline__ float norm3(V3 a) {
  float acc = __fmul_rn(a.x, a.x);
  acc = __fmaf_rn(a.y, a.y, acc);
  acc = __fmaf_rn(a.z, a.z, acc);
  return __fsqrt_rn(acc);
}
// a.pow(2).sum(-1).sqrt()
__device__ __forceinline__ float len3(V3 a) { return __fsqrt_rn(dot3(a, a)); }

// [p, q): entries of the (source-sorted) adjacency row [r0, r1) whose source equals s
__device__ __forceinline__ void equal_range(const int64_t* __restrict__ asrc, int64_t r0,
                                            int64_t r1, int64_t s, int64_t& p, int64_t& q) {
  int64_t lo = r0, hi = r1;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (asrc[m] < s) lo = m + 1;
    else hi = m;
  }
  p = lo;
  hi = r1;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (asrc[m] <= s) lo = m + 1;
    else hi = m;
  }
  q = lo;
}

// First backward of theta = atan2(b, a), a = u.v, b = |c|, c = u x v, scaled by g:
//   d theta = (a db - b da) / (a^2 + b^2);  da/du = v, da/dv = u;
//   db/du = v x c^, db/dv = c^ x u (c^ = c / b; 0 when b = 0, as torch's norm backward).
// gu = g dtheta/du, gv = g dtheta/dv; zero for g == 0.
__device__ __forceinline__ void angle_bwd(V3 u, V3 v, float g, V3& gu_out, V3& gv_out) {
  float gux = 0.f, guy = 0.f, guz = 0.f, gvx = 0.f, gvy = 0.f, gvz = 0.f;
  if (g != 0.f) {
    const V3 c = cross3(u, v);
    const float b = norm3(c), a = dot3(u, v);
    const float den = a * a + b * b;
    const float ga = -g * b / den, gb = g * a / den;
    gux = ga * v.x; guy = ga * v.y; guz = ga * v.z;
    gvx = ga * u.x; gvy = ga * u.y; gvz = ga * u.z;
    if (b > 0.f) {
      const V3 ch{c.x / b, c.y / b, c.z / b};
      gux += gb * (v.y * ch.z - v.z * ch.y);
      guy += gb * (v.z * ch.x - v.x * ch.z);
      guz += gb * (v.x * ch.y - v.y * ch.x);
      gvx += gb * (ch.y * u.z - ch.z * u.y);
      gvy += gb * (ch.z * u.x - ch.x * u.z);
      gvz += gb * (ch.x * u.y - ch.y * u.x);
    }
  }
  gu_out = V3{gux, guy, guz};
  gv_out = V3{gvx, gvy, gvz};
}

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 dd3(V3 a) { return D3{(double)a.x, (double)a.y, (double)a.z}; }
__device__ __forceinline__ D3 dxf(D3 a, D3 b) {
  return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 dadd(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 dscale(double s, D3 a) { return D3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ void st3(float* r, D3 a) {
  r[0] = (float)a.x; r[1] = (float)a.y; r[2] = (float)a.z;
}

// Second backward of the angle: forward mode (value + tangent) of angle_bwd along (du, dv), in
// double.  Returns gg = du.dtheta/du + dv.dtheta/dv; hu, hv = g Hess(theta) (du, dv), the
// directional derivatives of angle_bwd's gu, gv.  Dead cases as the first backward: b = 0 drops
// the c^ terms and their tangents, g == 0 leaves hu = hv = 0 (gg is still returned).
__device__ __forceinline__ double angle_bwd2(D3 u, D3 v, D3 du, D3 dv, double g, D3& hu_out,
                                             D3& hv_out) {
  const D3 c = dxf(u, v), dc = dadd(dxf(du, v), dxf(u, dv));
  const double b = sqrt(ddot(c, c)), a = ddot(u, v);
  const double da = ddot(du, v) + ddot(u, dv);
  const double db = b > 0.0 ? ddot(c, dc) / b : 0.0;
  const double den = a * a + b * b;
  D3 hu{0.0, 0.0, 0.0}, hv{0.0, 0.0, 0.0};
  double gg = 0.0;
  if (den > 0.0) {
    gg = (a * db - b * da) / den;
    if (g != 0.0) {
      const double dden = 2.0 * (a * da + b * db);
      const double ga = -g * b / den, gb = g * a / den;
      const double dga = -g * (db / den - b * dden / (den * den));
      const double dgb = g * (da / den - a * dden / (den * den));
      hu = dadd(dscale(dga, v), dscale(ga, dv));
      hv = dadd(dscale(dga, u), dscale(ga, du));
      if (b > 0.0) {
        const D3 ch = dscale(1.0 / b, c);
        const D3 dch = dadd(dscale(1.0 / b, dc), dscale(-db / (b * b), c));
        hu = dadd(hu, dadd(dscale(dgb, dxf(v, ch)),
                           dscale(gb, dadd(dxf(dv, ch), dxf(v, dch)))));
        hv = dadd(hv, dadd(dscale(dgb, dxf(ch, u)),
                           dscale(gb, dadd(dxf(dch, u), dxf(ch, du)))));
      }
    }
  }
  hu_out = hu;
  hv_out = hv;
  return gg;
}

inline int triplet_grid_for(int64_t n) {
  int64_t g = ceil_div(n, 256);
  const int64_t cap = (int64_t)device_cu_count() * 16;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace
}  // namespace gmp
