// The per-triplet and per-edge arithmetic of K11's geometry, the only home of its formulas: the
// node-form kernels (gmp_triplet.hip: u, v from pos) and the vector-form kernels
// (gmp_triplet_pbc.hip: u, v from the per-edge vectors of a periodic graph) call these helpers and
// write none of their own, so a graph with zero shifts gives the same bits in both forms.
// The forward helpers (dist_len3, dot3_sum, torsion_len3, torsion_candidate, cross3, norm3) state
// their roundings explicitly, as fma chains or under `fp contract(off)`: no forward value depends
// on what the compiler's contraction makes of a kernel.  They follow the reference's torch CPU
// evaluation except in the two lengths, which keep the roundings this project has always
// produced: dist is fma(y, y, x x) + z z and the torsion's |u| is fma(x, x, y y) + z z, where
// torch's `.pow(2).sum(-1)` is ((0 + x x) + y y) + z z.
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
// (a * b).sum(-1): every product rounded, then ((+0 + xx) + yy) + zz.  The reduction starts from
// +0, so an all-(-0) sum is +0 (atan2(0, +0) = 0, not pi, for a degenerate self-loop vector).
__device__ __forceinline__ float dot3_sum(V3 a, V3 b) {
#pragma clang fp contract(off)
  const float xx = a.x * b.x, yy = a.y * b.y, zz = a.z * b.z;
  return ((0.f + xx) + yy) + zz;
}
// a.norm(dim=-1)
__device__ __forceinline__ float norm3(V3 a) {
  float acc = __fmul_rn(a.x, a.x);
  acc = __fmaf_rn(a.y, a.y, acc);
  acc = __fmaf_rn(a.z, a.z, acc);
  return __fsqrt_rn(acc);
}
// dist of an edge: sqrt(fma(y, y, x x) + z z)
__device__ __forceinline__ float dist_len3(V3 a) {
#pragma clang fp contract(off)
  const float xx = a.x * a.x, zz = a.z * a.z;
  return __fsqrt_rn(__builtin_fmaf(a.y, a.y, xx) + zz);
}
// |u| of the torsion: sqrt(fma(x, x, y y) + z z)
__device__ __forceinline__ float torsion_len3(V3 a) {
#pragma clang fp contract(off)
  const float yy = a.y * a.y, zz = a.z * a.z;
  return __fsqrt_rn(__builtin_fmaf(a.x, a.x, yy) + zz);
}

// One candidate w of the torsion of (u, v): plane1 = u x v, dji = torsion_len3(u), plane2 = u x w,
// a = plane1.plane2, b = (plane1 x plane2).u / |u|; atan2(b, a) mapped to (0, 2 pi].
constexpr float kTwoPi = 6.283185307179586f;
__device__ __forceinline__ float torsion_candidate(V3 u, V3 plane1, float dji, V3 w) {
#pragma clang fp contract(off)
  const V3 plane2 = cross3(u, w);
  const float a = dot3_sum(plane1, plane2);
  const float b = dot3_sum(cross3(plane1, plane2), u) / dji;
  float t1 = atan2f(b, a);
  if (t1 <= 0.f) t1 = t1 + kTwoPi;
  return t1;
}
// torch_scatter min over the candidates: identity FLT_MAX, NaN never wins
constexpr float kNoTorsion = 3.402823466e38f;

// The backward helpers below are checked against fp64, not bit for bit, and leave the products
// and sums of dot3 / len3 (and their own) to the compiler's contraction.
__device__ __forceinline__ float dot3(V3 a, V3 b) {
  return __fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(a.x, b.x)), __fmul_rn(a.y, b.y)),
                   __fmul_rn(a.z, b.z));
}
__device__ __forceinline__ float len3(V3 a) { return __fsqrt_rn(dot3(a, a)); }
__device__ __forceinline__ V3 neg3(V3 a) { return V3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 acc3(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 xf(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ void st3(float* r, V3 a) {
  r[0] = a.x; r[1] = a.y; r[2] = a.z;
}

// The largest local edge lo of a fill block with s_off[lo] <= t (s_off: the block's nE + 1
// triplet offsets staged in LDS; s_off[0] <= t < s_off[nE])
__device__ __forceinline__ int find_local_edge(const int64_t* s_off, int nE, int64_t t) {
  int lo = 0, hi = nE;
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (s_off[m] <= t) lo = m;
    else hi = m;
  }
  return lo;
}

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

// Reverse mode of one torsion candidate t1 = atan2(b, a) scaled by g, with u = vec_ji, v the
// triplet's and w the winner's vector (the 2 pi shift has unit derivative):
//   P = u x v, Q = u x w, a = P.Q, R = P x Q, c = R.u, L = |u|, b = c / L
//   ga = -g b / (a^2 + b^2), gb = g a / (a^2 + b^2), gc = gb / L, gL = -gb c / L^2;
//   gu = gL u / L + gc R;  gR = gc u;  gP = Q x gR + ga Q;  gQ = gR x P + ga P;
//   gu += v x gP + w x gQ;  gv = gP x u;  gw = gQ x u.
// Dead cases, zero outputs: g == 0, a^2 + b^2 == 0 (an exactly collinear triplet, a candidate
// exactly parallel to u) and |u| == 0.
__device__ __forceinline__ void torsion_bwd(V3 u, V3 v, V3 w, float g, V3& gu, V3& gv, V3& gw) {
  const V3 z{0.f, 0.f, 0.f};
  gu = z; gv = z; gw = z;
  if (g == 0.f) return;
  const V3 P = cross3(u, v), Q = cross3(u, w), R = cross3(P, Q);
  const float a = dot3(P, Q), c = dot3(R, u), L = len3(u);
  if (!(L > 0.f)) return;
  const float b = c / L;
  const float den = a * a + b * b;
  if (!(den > 0.f)) return;
  const float ga = -g * b / den, gb = g * a / den;
  const float gc = gb / L, gL = -gb * c / (L * L);
  gu = V3{gL * u.x / L + gc * R.x, gL * u.y / L + gc * R.y, gL * u.z / L + gc * R.z};
  const V3 gR{gc * u.x, gc * u.y, gc * u.z};
  V3 gP = xf(Q, gR), gQ = xf(gR, P);
  gP = V3{gP.x + ga * Q.x, gP.y + ga * Q.y, gP.z + ga * Q.z};
  gQ = V3{gQ.x + ga * P.x, gQ.y + ga * P.y, gQ.z + ga * P.z};
  gu = acc3(gu, acc3(xf(v, gP), xf(w, gQ)));
  gv = xf(gP, u);
  gw = xf(gQ, u);
}

// First backward of dist = |d| scaled by g: the row r = g d / |d| with
// |d| = sqrt(fma(z, z, x x + y y)) and, in node form, its negative r_neg for the other end of the
// edge; zero for g == 0 and |d| == 0.
__device__ __forceinline__ void dist_bwd_row(V3 d, float g, float* r, float* r_neg = nullptr) {
#pragma clang fp contract(off)
  const float len = __fsqrt_rn(__builtin_fmaf(d.z, d.z, d.x * d.x + d.y * d.y));
  const float s = (g != 0.f && len > 0.f) ? g / len : 0.f;
  r[0] = s * d.x; r[1] = s * d.y; r[2] = s * d.z;
  if (r_neg) {
    r_neg[0] = -(s * d.x); r_neg[1] = -(s * d.y); r_neg[2] = -(s * d.z);
  }
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

// Second backward of dist: returns dlen = d.dd / |d| and h = g Hess(|d|) dd, the directional
// derivative of dist_bwd_row along dd, in double.  Dead cases as dist_bwd_row (dlen is still
// returned for g == 0).
__device__ __forceinline__ double dist_bwd2(D3 d, D3 dd, double g, D3& h) {
  const double len = sqrt(ddot(d, d));
  const double dlen = len > 0.0 ? ddot(d, dd) / len : 0.0;
  h = D3{0.0, 0.0, 0.0};
  if (g != 0.0 && len > 0.0) h = dadd(dscale(g / len, dd), dscale(-g * dlen / (len * len), d));
  return dlen;
}

inline int triplet_grid_for(int64_t n) {
  int64_t g = ceil_div(n, 256);
  const int64_t cap = (int64_t)device_cu_count() * 16;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

}  // namespace
}  // namespace gmp
