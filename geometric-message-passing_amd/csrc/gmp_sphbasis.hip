// K18 / K18d: the spherical bases of SphereNet (models/layers/spherenet_layer.py: dist_emb,
// angle_emb, torsion_emb) and DimeNet++ (PyG 2.3.1 DimeNetPlusPlus: BesselBasisLayer,
// SphericalBasisLayer) without the per-triplet embeddings in HBM.  One set of kernels, each
// instantiated twice:
//
//   kCut (per edge):        false = SphereNet, true = DimeNet++
//   kTorsion (per triplet): true = SphereNet (angle and torsion features), false = DimeNet++
//                           (angle features only)
//
// Per edge (gmp_sph_edge_basis_*, gmp_dime_edge_basis_*): rbf[q] = envelope(x) sin(freq_q x) and
// jb[l, q] = N_lq j_l(z_lq x), x = d / cutoff.  With kCut the envelope is also multiplied into
// jb (PyG's sbf), and values and gradients are exactly zero at and beyond the cutoff (PyG's
// [x < 1]).  The reference evaluates j_l by its closed form (sin / cos over powers of x), which
// cancels catastrophically for small arguments: j_6 at x = 0.05 comes out as -0.6 in fp32 where
// the value is ~1e-9.  Here j_l is a power series below x = l + 1 (all terms after the first few
// decrease, no cancellation) and the upward recurrence from j_0, j_1 above (stable for x > l).
// E is small next to T, so the per-edge arithmetic runs in double and is rounded once.
//
// Per triplet (gmp_sph_triplet_proj_*, gmp_dime_triplet_proj_*): the n k angle features
// jb[kj][l, q] Y_l0(theta) and, with kTorsion, the n^2 k torsion features jb[kj][b, q]
// Yflat[a n + b](theta, phi) are formed in LDS from the gathered jb row and the harmonics of the
// triplet, and multiplied at once into the first projections of every layer: S (L, T, ba),
// P (L, T, bt).  The reference's layout is kept: per l the harmonics are ordered m = 0, 1..l
// (cos), -l..-1 (sin), and the view(-1, n, n, 1) of torsion_emb pairs Bessel order b with flat
// harmonic a n + b.  Without kTorsion only the n values Y_l0 are formed and staged (row l).
#include <algorithm>

#include "gmp_common.h"

namespace gmp {
namespace {

constexpr int kTile = 64;        // triplets per tile (one per lane)
constexpr int kLd = kTile + 1;   // LDS row stride of the staged [feature][triplet] planes
constexpr int kOC = 8;           // output columns per accumulator chunk
constexpr int kEdgeT = 256;
constexpr size_t kLdsCap = 60 * 1024;
// Grid caps of the weight-gradient kernel; they fix the order of the partial sums.  Without the
// torsion features its blocks are one wave at the default basis (n k = 42 features <= 64), so the
// grid is what fills the chip: 4096 blocks (0.69 ms at 3.5M triplets; 2.29 ms at 512).
constexpr int kProjBwdBlocks = 512;
constexpr int kProjBwdBlocksAngleOnly = 4096;

// j_l(x) for x > 0
__device__ double sph_jl(int l, double x) {
  if (x < (double)(l + 1)) {
    double pre = 1.0;  // x^l / (2l + 1)!!
    for (int i = 1; i <= l; ++i) pre *= x / (double)(2 * i + 1);
    const double h = -0.5 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k <= 30; ++k) {
      term *= h / ((double)k * (double)(2 * l + 2 * k + 1));
      sum += term;
    }
    return pre * sum;
  }
  double s, c;
  sincos(x, &s, &c);
  double j0 = s / x;
  if (l == 0) return j0;
  double j1 = (j0 - c) / x;
  for (int i = 1; i < l; ++i) {
    const double j2 = (double)(2 * i + 1) / x * j1 - j0;
    j0 = j1;
    j1 = j2;
  }
  return j1;
}

// j_l'(x) = j_{l-1}(x) - (l + 1) / x j_l(x);  j_0' = -j_1
__device__ double sph_jl_prime(int l, double x) {
  if (l == 0) return -sph_jl(1, x);
  return sph_jl(l - 1, x) - (double)(l + 1) / x * sph_jl(l, x);
}

__device__ double ipow(double x, int n) {
  double r = 1.0;
  for (int i = 0; i < n; ++i) r *= x;
  return r;
}

// envelope(x) = 1/x + a x^(p-1) + b x^p + c x^(p+1), its derivative and, where asked for, its
// second derivative (a power whose coefficient is zero is not evaluated: p - 3 < 0 at p = 2)
__device__ void env_eval(int exponent, double x, double* v, double* dv, double* d2v = nullptr) {
  const int p = exponent + 1;
  const double a = -(double)(p + 1) * (p + 2) / 2.0, b = (double)p * (p + 2),
               c = -(double)p * (p + 1) / 2.0;
  const double x0 = ipow(x, p - 1);
  const double x1 = x0 * x, x2 = x1 * x;
  *v = 1.0 / x + a * x0 + b * x1 + c * x2;
  const double xm = p >= 2 ? ipow(x, p - 2) : 0.0;
  *dv = -1.0 / (x * x) + a * (double)(p - 1) * xm + b * (double)p * x0 + c * (double)(p + 1) * x1;
  if (d2v) {
    const double xmm = p >= 3 ? ipow(x, p - 3) : 0.0;
    *d2v = 2.0 / (x * x * x) + a * (double)((p - 1) * (p - 2)) * xmm +
           b * (double)(p * (p - 1)) * xm + c * (double)((p + 1) * p) * x0;
  }
}

// thread per (edge, column), columns [0, k) = rbf, [k, k + n k) = jb
template <bool kCut>
__global__ __launch_bounds__(kEdgeT) void edge_basis_fwd(
    const float* __restrict__ dist, int64_t E, float cutoff, int exponent,
    const float* __restrict__ freq, int k, const float* __restrict__ zeros,
    const float* __restrict__ norm, int nk, float* __restrict__ rbf, float* __restrict__ jb) {
  const int cols = k + nk;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= E * cols) return;
  const int64_t e = i / cols;
  const int c = (int)(i - e * cols);
  const double x = (double)dist[e] / (double)cutoff;
  float out = 0.f;
  if (!kCut || x < 1.0) {
    double v = 0.0, dv = 0.0;
    if (kCut || c < k) env_eval(exponent, x, &v, &dv);
    if (c < k) {
      out = (float)(v * sin((double)freq[c] * x));
    } else {
      const int lq = c - k;
      const double scale = kCut ? v * (double)norm[lq] : (double)norm[lq];
      out = (float)(scale * sph_jl(lq / k, (double)zeros[lq] * x));
    }
  }
  if (c < k) rbf[e * k + c] = out;
  else jb[e * nk + (c - k)] = out;
}

// thread per edge: g_dist[e]; the freq gradient of the block's edges is tree-summed in LDS in
// a fixed order into one partial row per block.  With kCut an edge at or beyond the cutoff is
// dead: it is evaluated at x = 0.5 to stay finite and contributes exact zeros.
template <bool kCut>
__global__ __launch_bounds__(kEdgeT) void edge_basis_bwd(
    const float* __restrict__ dist, int64_t E, float cutoff, int exponent,
    const float* __restrict__ freq, int k, const float* __restrict__ zeros,
    const float* __restrict__ norm, int nk, const float* __restrict__ g_rbf,
    const float* __restrict__ g_jb, float* __restrict__ g_dist,
    float* __restrict__ freq_partials) {
  __shared__ float red[kEdgeT];
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool in_range = e < E;
  const double xr = in_range ? (double)dist[e] / (double)cutoff : 1.0;
  const bool live = in_range && (!kCut || xr < 1.0);
  const double x = kCut && !live ? 0.5 : xr;
  const double inv_c = 1.0 / (double)cutoff;
  double env = 0.0, denv = 0.0;
  env_eval(exponent, x, &env, &denv);
  double gd = 0.0;
  for (int q = 0; q < k; ++q) {
    float contrib = 0.f;
    if (live && g_rbf) {
      const double f = (double)freq[q], g = (double)g_rbf[e * k + q];
      double s, c;
      sincos(f * x, &s, &c);
      gd += g * (denv * s + env * f * c) * inv_c;
      contrib = (float)(g * env * x * c);
    }
    red[threadIdx.x] = contrib;
    __syncthreads();
    for (int w = kEdgeT / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) freq_partials[(int64_t)blockIdx.x * k + q] = red[0];
    __syncthreads();
  }
  if (!in_range) return;
  if (live && g_jb) {
    for (int lq = 0; lq < nk; ++lq) {
      const double z = (double)zeros[lq];
      const int l = lq / k;
      if constexpr (kCut) {
        gd += (double)g_jb[e * nk + lq] * (double)norm[lq] * inv_c *
              (denv * sph_jl(l, z * x) + env * z * sph_jl_prime(l, z * x));
      } else {
        gd += (double)g_jb[e * nk + lq] * (double)norm[lq] * z * inv_c * sph_jl_prime(l, z * x);
      }
    }
  }
  g_dist[e] = live ? (float)gd : 0.f;
}

// j_l''(y) = -(2 / y) j_l'(y) - (1 - l (l + 1) / y^2) j_l(y)  (the spherical Bessel equation)
__device__ double sph_jl_second(int l, double y, double j, double dj) {
  return -(2.0 / y) * dj - (1.0 - (double)(l * (l + 1)) / (y * y)) * j;
}

// Second backward of the edge basis: thread per edge.  The first backward maps (g_rbf, g_jb)
// to (g_dist, g_freq); with the cotangents a_dist (E) and a_freq (k) of those this writes
// gg_rbf, gg_jb (the gradients w.r.t. g_rbf, g_jb) and h_dist, and the block's h_freq partial
// row, tree-summed in LDS in a fixed order as edge_basis_bwd.  With s = sin(f x), c = cos(f x):
//   gg_rbf[q] = a_d (env' s + env f c) / cutoff + a_f[q] env x c
//   gg_jb[lq] = a_d N (env' j + env z j') / cutoff            (kCut; N z j' / cutoff without)
//   h_dist    = a_d [sum_q g_rbf (env'' s + 2 env' f c - env f^2 s)
//                    + sum_lq g_jb N (env'' j + 2 env' z j' + env z^2 j'')] / cutoff^2
//               + sum_q a_f[q] g_rbf (env' x c + env c - env f x s) / cutoff
//   h_freq[q] = sum_e g_rbf [a_d (env' x c + env c - env f x s) / cutoff - a_f[q] env x^2 s]
// All in double, rounded once.  With kCut a dead edge writes exact zeros everywhere.
template <bool kCut>
__global__ __launch_bounds__(kEdgeT) void edge_basis_bwd2(
    const float* __restrict__ dist, int64_t E, float cutoff, int exponent,
    const float* __restrict__ freq, int k, const float* __restrict__ zeros,
    const float* __restrict__ norm, int nk, const float* __restrict__ g_rbf,
    const float* __restrict__ g_jb, const float* __restrict__ a_dist,
    const float* __restrict__ a_freq, float* __restrict__ gg_rbf, float* __restrict__ gg_jb,
    float* __restrict__ h_dist, float* __restrict__ freq_partials) {
  __shared__ float red[kEdgeT];
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool in_range = e < E;
  const double xr = in_range ? (double)dist[e] / (double)cutoff : 1.0;
  const bool live = in_range && (!kCut || xr < 1.0);
  const double x = kCut && !live ? 0.5 : xr;
  const double inv_c = 1.0 / (double)cutoff;
  double env = 0.0, denv = 0.0, d2env = 0.0;
  env_eval(exponent, x, &env, &denv, &d2env);
  const double ad = (live && a_dist) ? (double)a_dist[e] : 0.0;
  double hd = 0.0;
  for (int q = 0; q < k; ++q) {
    float contrib = 0.f, gg = 0.f;
    if (live) {
      const double f = (double)freq[q];
      const double g = g_rbf ? (double)g_rbf[e * k + q] : 0.0;
      const double af = a_freq ? (double)a_freq[q] : 0.0;
      double s, c;
      sincos(f * x, &s, &c);
      const double m = denv * x * c + env * c - env * f * x * s;
      gg = (float)(ad * (denv * s + env * f * c) * inv_c + af * env * x * c);
      hd += ad * g * (d2env * s + 2.0 * denv * f * c - env * f * f * s) * inv_c * inv_c +
            af * g * m * inv_c;
      contrib = (float)(g * (ad * m * inv_c - af * env * x * x * s));
    }
    if (in_range) gg_rbf[e * k + q] = gg;
    red[threadIdx.x] = contrib;
    __syncthreads();
    for (int w = kEdgeT / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) freq_partials[(int64_t)blockIdx.x * k + q] = red[0];
    __syncthreads();
  }
  if (!in_range) return;
  for (int lq = 0; lq < nk; ++lq) {
    float gg = 0.f;
    if (live) {
      const double z = (double)zeros[lq], N = (double)norm[lq];
      const int l = lq / k;
      const double y = z * x;
      const double j = sph_jl(l, y), dj = sph_jl_prime(l, y);
      const double d2j = sph_jl_second(l, y, j, dj);
      const double g = g_jb ? (double)g_jb[e * nk + lq] : 0.0;
      if constexpr (kCut) {
        gg = (float)(ad * N * (denv * j + env * z * dj) * inv_c);
        hd += ad * g * N * (d2env * j + 2.0 * denv * z * dj + env * z * z * d2j) * inv_c * inv_c;
      } else {
        gg = (float)(ad * N * z * dj * inv_c);
        hd += ad * g * N * z * z * d2j * inv_c * inv_c;
      }
    }
    gg_jb[e * nk + lq] = gg;
  }
  h_dist[e] = live ? (float)hd : 0.f;
}

// the staged harmonics: row of Y_l0, and the number of rows
template <bool kTorsion>
__host__ __device__ constexpr int y_row(int l) {
  return kTorsion ? l * l : l;
}
template <bool kTorsion>
__host__ __device__ constexpr int y_planes(int n) {
  return kTorsion ? n * n : n;
}

// element (t, o) of the (L, T, b) layout of S / P and their gradients, o = layer * b + j
__device__ __forceinline__ int64_t proj_index(int o, int64_t t, int64_t T, int b) {
  return ((int64_t)(o / b) * T + t) * b + o % b;
}

// The n^2 real harmonics of one direction, flat index l^2 + p with p = 0 (m = 0), 1..l (cos m
// = p), l + 1..2l (sin m = 2l + 1 - p).  Y_l^m = pref[l^2 + p] P_l^m(cos theta) {C_m, S_m} with
// C_m + i S_m = (sin theta e^{i phi})^m and P_l^m the polynomial part of the associated
// Legendre function (the sin^m theta factor lives in C_m, S_m), built by the recurrences of
// the reference's generator; pref carries the sqrt(2) of m != 0.
// Without kTorsion only m = 0 runs (the Legendre recurrence; phi is not read) and Y_l0 is row l.
// kGrad: instead of storing Y, returns sum_idx gY[idx] dY[idx]/dtheta and /dphi.
template <bool kGrad, bool kTorsion>
__device__ void sph_harmonics(int n, float theta, float phi, const float* __restrict__ pref,
                              float* Y, int stride, float* g_theta, float* g_phi) {
  float st, ct, sp, cp;
  sincosf(theta, &st, &ct);
  sincosf(phi, &sp, &cp);
  const float x = st * cp, y = st * sp;
  const float dxt = ct * cp, dyt = ct * sp;  // d/dtheta; d/dphi of (x, y) is (-y, x)
  float C = 1.f, S = 0.f, dCt = 0.f, dSt = 0.f;
  float pmm = 1.f;  // P_m^m = (-1)^m (2m - 1)!!
  float gt = 0.f, gp = 0.f;
  for (int m = 0; m < (kTorsion ? n : 1); ++m) {
    if (m > 0) {
      const float C1 = x * C - y * S, S1 = x * S + y * C;
      const float dC1 = dxt * C + x * dCt - dyt * S - y * dSt;
      const float dS1 = dxt * S + x * dSt + dyt * C + y * dCt;
      C = C1, S = S1, dCt = dC1, dSt = dS1;
      pmm *= (float)(1 - 2 * m);
    }
    float p2 = 0.f, dp2 = 0.f;         // P_{l-2}^m and d/dz
    float p1 = 0.f, dp1 = 0.f;         // P_{l-1}^m
    for (int l = m; l < n; ++l) {
      float p, dp;
      if (l == m) {
        p = pmm, dp = 0.f;
      } else if (l == m + 1) {
        p = (float)(2 * m + 1) * ct * p1, dp = (float)(2 * m + 1) * p1;
      } else {
        const float inv = 1.f / (float)(l - m);
        p = ((float)(2 * l - 1) * ct * p1 - (float)(l + m - 1) * p2) * inv;
        dp = ((float)(2 * l - 1) * (p1 + ct * dp1) - (float)(l + m - 1) * dp2) * inv;
      }
      p2 = p1, dp2 = dp1, p1 = p, dp1 = dp;
      const int base = l * l;
      if (m == 0) {
        const float f = pref[base];
        const int i0 = y_row<kTorsion>(l);
        if (kGrad) gt += Y[i0 * stride] * f * dp * (-st);
        else Y[i0 * stride] = f * p;
      } else {
        const int ic = base + m, is = base + 2 * l + 1 - m;
        const float fc = pref[ic], fs = pref[is];
        if (kGrad) {
          const float gc = Y[ic * stride], gs = Y[is * stride];
          gt += gc * fc * (dCt * p - C * dp * st) + gs * fs * (dSt * p - S * dp * st);
          gp += gc * fc * (-(float)m * S) * p + gs * fs * ((float)m * C) * p;
        } else {
          Y[ic * stride] = fc * C * p;
          Y[is * stride] = fs * S * p;
        }
      }
    }
  }
  if (kGrad) *g_theta = gt, *g_phi = gp;
}

// Stage one tile: jbL[c * kLd + r] = jb[idx_kj[t0 + r], c] (coalesced rows), YL[idx * kLd + r].
// kjL (kTile ints) is scratch.  All threads of the block take part; ends with a barrier.
template <bool kTorsion>
__device__ void stage_tile(int64_t t0, int64_t T, int64_t E, int n, int nk,
                           const float* __restrict__ jb,
                           const float* __restrict__ angle, const float* __restrict__ torsion,
                           const int64_t* __restrict__ idx_kj, const float* __restrict__ pref,
                           float* jbL, float* YL, int64_t* kjL) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid < kTile) {
    const int64_t kj = t0 + tid < T ? idx_kj[t0 + tid] : -1;
    kjL[tid] = kj < E ? kj : -1;  // an index outside the edges reads as a zero row
  }
  __syncthreads();
  for (int i = tid; i < kTile * nk; i += nt) {
    const int r = i / nk, c = i - r * nk;
    const int64_t kj = kjL[r];
    jbL[c * kLd + r] = kj >= 0 ? jb[kj * nk + c] : 0.f;
  }
  if (tid < kTile) {
    if (t0 + tid < T) {
      sph_harmonics<false, kTorsion>(n, angle[t0 + tid], kTorsion ? torsion[t0 + tid] : 0.f, pref,
                                     YL + tid, kLd, nullptr, nullptr);
    } else {
      for (int i = 0; i < y_planes<kTorsion>(n); ++i) YL[i * kLd + tid] = 0.f;
    }
  }
  __syncthreads();
}

// one wave per tile, lane = triplet.  w1t (n k, oa_ld), w2t (n^2 k, ot_ld): feature-major,
// columns o = layer * b + j, leading dimensions padded to a multiple of kOC with zeros.
// The arguments that only kTorsion reads (torsion, w2t, Ot, ot_ld, bt, P) come last, here and in
// the kernels below: the angle-only instantiation then loads a prefix of the argument block and
// nothing of the rest (the order changes its prologue, and with it the measured time by 2-6 %).
template <bool kTorsion>
__global__ __launch_bounds__(kTile) void triplet_proj_fwd(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ w1t, int Oa, int oa_ld, int ba,
    float* __restrict__ S, const float* __restrict__ torsion, const float* __restrict__ w2t,
    int Ot, int ot_ld, int bt, float* __restrict__ P) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile<kTorsion>(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    const int64_t t = t0 + lane;
    for (int o0 = 0; o0 < Oa; o0 += kOC) {
      float acc[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
      for (int l = 0; l < n; ++l) {
        const float y = YL[y_row<kTorsion>(l) * kLd + lane];
        for (int q = 0; q < k; ++q) {
          const int f = l * k + q;
          const float e = jbL[f * kLd + lane] * y;
          const float* w = w1t + (int64_t)f * oa_ld + o0;
#pragma unroll
          for (int u = 0; u < kOC; ++u) acc[u] = fmaf(w[u], e, acc[u]);
        }
      }
      if (t < T) {
#pragma unroll
        for (int u = 0; u < kOC; ++u) {
          const int o = o0 + u;
          if (o < Oa) S[proj_index(o, t, T, ba)] = acc[u];
        }
      }
    }
    if constexpr (kTorsion) {
      for (int o0 = 0; o0 < Ot; o0 += kOC) {
        float acc[kOC];
#pragma unroll
        for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
        for (int ab = 0; ab < n * n; ++ab) {
          const float y = YL[ab * kLd + lane];
          const int b = ab % n;
          for (int q = 0; q < k; ++q) {
            const float e = jbL[(b * k + q) * kLd + lane] * y;
            const float* w = w2t + ((int64_t)ab * k + q) * ot_ld + o0;
#pragma unroll
            for (int u = 0; u < kOC; ++u) acc[u] = fmaf(w[u], e, acc[u]);
          }
        }
        if (t < T) {
#pragma unroll
          for (int u = 0; u < kOC; ++u) {
            const int o = o0 + u;
            if (o < Ot) P[proj_index(o, t, T, bt)] = acc[u];
          }
        }
      }
    }
  }
}

// the materialising form: angle_emb (T, n k) and, with kTorsion, torsion_emb (T, n^2 k)
template <bool kTorsion>
__global__ __launch_bounds__(kTile) void triplet_emb(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, float* __restrict__ aemb,
    const float* __restrict__ torsion, float* __restrict__ temb) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile<kTorsion>(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    for (int r = 0; r < kTile && t0 + r < T; ++r) {
      for (int f = lane; f < nk; f += kTile)
        aemb[(t0 + r) * nk + f] = jbL[f * kLd + r] * YL[y_row<kTorsion>(f / k) * kLd + r];
      if constexpr (kTorsion) {
        const int nnk = n * nk;
        for (int f = lane; f < nnk; f += kTile) {
          const int ab = f / k, q = f - ab * k;
          temb[(t0 + r) * nnk + f] = jbL[((ab % n) * k + q) * kLd + r] * YL[ab * kLd + r];
        }
      }
    }
  }
}

// Weight gradients: block b sums its contiguous range of tiles, thread = feature (angle
// features first, then with kTorsion the torsion features), blockIdx.y = chunk of kOC output
// columns; triplets are added in index order.  One partial row [g_w1t | g_w2t] per block.
template <bool kTorsion>
__global__ void triplet_proj_wgrad(
    int64_t T, int64_t E, int n, int k, int64_t tiles_per_block, const float* __restrict__ jb,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ gS, int Oa, int oa_ld, int ba,
    float* __restrict__ partials, const float* __restrict__ torsion,
    const float* __restrict__ gP, int Ot, int ot_ld, int bt) {
  constexpr int kGroups = kTorsion ? 2 : 1;  // weight matrices
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  __shared__ float gL[kGroups][kTile][kOC];
  const int nk = n * k, nnk = kTorsion ? n * nk : 0;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  const int tid = threadIdx.x;
  const int o0 = blockIdx.y * kOC;
  const int f = tid;
  const bool is_a = f < nk, is_t = kTorsion && f >= nk && f < nk + nnk;
  int jrow = 0, yrow = 0;
  if (is_a) {
    jrow = f, yrow = y_row<kTorsion>(f / k);
  } else if (is_t) {
    const int ft = f - nk, ab = ft / k;
    jrow = (ab % n) * k + (ft - ab * k), yrow = ab;
  }
  const int which = is_a ? 0 : kGroups - 1;
  // blockIdx.y runs over the chunks of the wider weight group; a single group owns them all
  const bool active = kTorsion ? (is_a && o0 < Oa) || (is_t && o0 < Ot) : is_a;
  float acc[kOC];
#pragma unroll
  for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_block;
  for (int64_t tile = tile0; tile < tile0 + tiles_per_block; ++tile) {
    const int64_t t0 = tile * kTile;
    if (t0 >= T) break;
    __syncthreads();
    stage_tile<kTorsion>(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    for (int i = tid; i < kGroups * kTile * kOC; i += blockDim.x) {
      const int w = i / (kTile * kOC), r = (i / kOC) % kTile, u = i % kOC;
      const int o = o0 + u;
      const int64_t t = t0 + r;
      float v = 0.f;
      if (t < T) {
        if (w == 0 && o < Oa) v = gS[proj_index(o, t, T, ba)];
        if (kTorsion && w == 1 && o < Ot) v = gP[proj_index(o, t, T, bt)];
      }
      gL[w][r][u] = v;
    }
    __syncthreads();
    if (active) {
      for (int r = 0; r < kTile; ++r) {
        const float e = jbL[jrow * kLd + r] * YL[yrow * kLd + r];
#pragma unroll
        for (int u = 0; u < kOC; ++u) acc[u] = fmaf(gL[which][r][u], e, acc[u]);
      }
    }
  }
  const int64_t width = (int64_t)nk * oa_ld + (int64_t)nnk * ot_ld;
  float* row = partials + (int64_t)blockIdx.x * width;
  if (is_a && (!kTorsion || o0 < oa_ld)) {
#pragma unroll
    for (int u = 0; u < kOC; ++u) row[(int64_t)f * oa_ld + o0 + u] = acc[u];
  } else if (is_t && o0 < ot_ld) {
#pragma unroll
    for (int u = 0; u < kOC; ++u)
      row[(int64_t)nk * oa_ld + (int64_t)(f - nk) * ot_ld + o0 + u] = acc[u];
  }
}

// Geometry gradients: lane = triplet; g_emb[f] = sum_o w[f, o] g[o] is folded at once into
// g_jb (per-triplet rows, summed per edge by the caller over the CSR of idx_kj) and g_Y, which
// the harmonics' derivatives turn into g_angle and, with kTorsion, g_torsion.
template <bool kTorsion>
__global__ __launch_bounds__(kTile) void triplet_proj_geom_bwd(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ w1t, int Oa, int oa_ld, int ba,
    const float* __restrict__ gS, float* __restrict__ g_jb_rows, float* __restrict__ g_angle,
    const float* __restrict__ torsion, const float* __restrict__ w2t, int Ot, int ot_ld, int bt,
    const float* __restrict__ gP, float* __restrict__ g_torsion) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k, ny = y_planes<kTorsion>(n);
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  float* gjL = YL + ny * kLd;
  float* gyL = gjL + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile<kTorsion>(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    const int64_t t = t0 + lane;
    for (int i = 0; i < nk; ++i) gjL[i * kLd + lane] = 0.f;
    for (int i = 0; i < ny; ++i) gyL[i * kLd + lane] = 0.f;
    for (int o0 = 0; o0 < Oa; o0 += kOC) {
      float g[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) {
        const int o = o0 + u;
        g[u] = (t < T && o < Oa) ? gS[proj_index(o, t, T, ba)] : 0.f;
      }
      for (int l = 0; l < n; ++l) {
        const int yl = y_row<kTorsion>(l);
        const float y = YL[yl * kLd + lane];
        float gy = 0.f;
        for (int q = 0; q < k; ++q) {
          const int f = l * k + q;
          const float* w = w1t + (int64_t)f * oa_ld + o0;
          float ge = 0.f;
#pragma unroll
          for (int u = 0; u < kOC; ++u) ge = fmaf(w[u], g[u], ge);
          gjL[f * kLd + lane] += ge * y;
          gy = fmaf(ge, jbL[f * kLd + lane], gy);
        }
        gyL[yl * kLd + lane] += gy;
      }
    }
    if constexpr (kTorsion) {
      for (int o0 = 0; o0 < Ot; o0 += kOC) {
        float g[kOC];
#pragma unroll
        for (int u = 0; u < kOC; ++u) {
          const int o = o0 + u;
          g[u] = (t < T && o < Ot) ? gP[proj_index(o, t, T, bt)] : 0.f;
        }
        for (int ab = 0; ab < ny; ++ab) {
          const float y = YL[ab * kLd + lane];
          const int b = ab % n;
          float gy = 0.f;
          for (int q = 0; q < k; ++q) {
            const float* w = w2t + ((int64_t)ab * k + q) * ot_ld + o0;
            float ge = 0.f;
#pragma unroll
            for (int u = 0; u < kOC; ++u) ge = fmaf(w[u], g[u], ge);
            gjL[(b * k + q) * kLd + lane] += ge * y;
            gy = fmaf(ge, jbL[(b * k + q) * kLd + lane], gy);
          }
          gyL[ab * kLd + lane] += gy;
        }
      }
    }
    if (t < T) {
      float gt, gp;
      sph_harmonics<true, kTorsion>(n, angle[t], kTorsion ? torsion[t] : 0.f, pref, gyL + lane,
                                    kLd, &gt, &gp);
      g_angle[t] = gt;
      if constexpr (kTorsion) g_torsion[t] = gp;
    }
    __syncthreads();
    for (int r = 0; r < kTile && t0 + r < T; ++r)
      for (int c = lane; c < nk; c += kTile) g_jb_rows[(t0 + r) * nk + c] = gjL[c * kLd + r];
  }
}

// ---- second backward of the angle-only projection (DimeNet++ energy-and-force training).
// The first backward maps gS to (g_w, g_sbe, g_angle); with their cotangents a_w (feature-major
// as w1t), a_sbe (E, n k), a_angle (T), each possibly null, and
//   sbf_t  = sbe[kj] * Y,   sdot_t = a_sbe[kj] * Y + sbe[kj] * Y' a_angle[t],
//   u_t    = sum_o w[., o] gS[o, t],   udot_t = sum_o a_w[., o] gS[o, t]
// the second backward is
//   gg_S[o, t]    = w[., o].sdot_t + a_w[., o].sbf_t                    (triplet_proj_bwd2_ggs)
//   h_w[f, o]     = sum_t gS[o, t] sdot_t[f]                            (triplet_proj_bwd2_wgrad)
//   h_sbe_rows[t] = udot_t * Y + u_t * Y' a_angle[t]                    (triplet_proj_bwd2_geom)
//   h_angle[t]    = sum_f (udot_t sbe Y' + u_t a_sbe[kj] Y' + a_angle[t] u_t sbe Y'').

// Y_l0 and its first two derivatives in theta from the Legendre recurrence in z = cos theta:
// dY/dtheta = -sin P', d2Y/dtheta2 = sin^2 P'' - cos P' (regular at 0 and pi).  Y2 may be null.
__device__ void legendre_y012(int n, float theta, const float* __restrict__ pref, float* Y,
                              float* Y1, float* Y2, int stride) {
  float st, ct;
  sincosf(theta, &st, &ct);
  float p2 = 0.f, d2 = 0.f, e2 = 0.f;  // P_{l-2}, P', P''
  float p1 = 0.f, d1 = 0.f, e1 = 0.f;  // P_{l-1}
  for (int l = 0; l < n; ++l) {
    float p, d, e;
    if (l == 0) {
      p = 1.f, d = 0.f, e = 0.f;
    } else if (l == 1) {
      p = ct, d = 1.f, e = 0.f;
    } else {
      const float inv = 1.f / (float)l, c1 = (float)(2 * l - 1), c2 = (float)(l - 1);
      p = (c1 * ct * p1 - c2 * p2) * inv;
      d = (c1 * (p1 + ct * d1) - c2 * d2) * inv;
      e = (c1 * (2.f * d1 + ct * e1) - c2 * e2) * inv;
    }
    p2 = p1, d2 = d1, e2 = e1, p1 = p, d1 = d, e1 = e;
    const float f = pref[l * l];
    Y[l * stride] = f * p;
    Y1[l * stride] = -f * st * d;
    if (Y2) Y2[l * stride] = f * (st * st * e - ct * d);
  }
}

// stage_tile<false> with the gathered a_sbe rows (zeros if null), Y' and, where Y2L is given,
// Y'' planes and the tile's a_angle (zeros if null).  Ends with a barrier.
__device__ void stage_tile2(int64_t t0, int64_t T, int64_t E, int n, int nk,
                            const float* __restrict__ jb, const float* __restrict__ a_jb,
                            const float* __restrict__ angle, const float* __restrict__ a_angle,
                            const int64_t* __restrict__ idx_kj, const float* __restrict__ pref,
                            float* jbL, float* ajL, float* YL, float* Y1L, float* Y2L, float* aaL,
                            int64_t* kjL) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid < kTile) {
    const int64_t kj = t0 + tid < T ? idx_kj[t0 + tid] : -1;
    kjL[tid] = kj < E ? kj : -1;
    aaL[tid] = (a_angle && t0 + tid < T) ? a_angle[t0 + tid] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < kTile * nk; i += nt) {
    const int r = i / nk, c = i - r * nk;
    const int64_t kj = kjL[r];
    jbL[c * kLd + r] = kj >= 0 ? jb[kj * nk + c] : 0.f;
    ajL[c * kLd + r] = (kj >= 0 && a_jb) ? a_jb[kj * nk + c] : 0.f;
  }
  if (tid < kTile) {
    if (t0 + tid < T) {
      legendre_y012(n, angle[t0 + tid], pref, YL + tid, Y1L + tid, Y2L ? Y2L + tid : nullptr,
                    kLd);
    } else {
      for (int i = 0; i < n; ++i) {
        YL[i * kLd + tid] = 0.f;
        Y1L[i * kLd + tid] = 0.f;
        if (Y2L) Y2L[i * kLd + tid] = 0.f;
      }
    }
  }
  __syncthreads();
}

// forward-shaped: one wave per tile, lane = triplet
__global__ __launch_bounds__(kTile) void triplet_proj_bwd2_ggs(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ a_jb, const float* __restrict__ angle,
    const float* __restrict__ a_angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ w1t,
    const float* __restrict__ a_w1t, int Oa, int oa_ld, int ba, float* __restrict__ ggS) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  __shared__ float aaL[kTile];
  const int nk = n * k;
  float* jbL = sm;
  float* ajL = jbL + nk * kLd;
  float* YL = ajL + nk * kLd;
  float* Y1L = YL + n * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile2(t0, T, E, n, nk, jb, a_jb, angle, a_angle, idx_kj, pref, jbL, ajL, YL, Y1L,
                nullptr, aaL, kjL);
    const int64_t t = t0 + lane;
    const float aa = aaL[lane];
    for (int o0 = 0; o0 < Oa; o0 += kOC) {
      float acc[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
      for (int l = 0; l < n; ++l) {
        const float y = YL[l * kLd + lane], y1a = Y1L[l * kLd + lane] * aa;
        for (int q = 0; q < k; ++q) {
          const int f = l * k + q;
          const float s = jbL[f * kLd + lane];
          const float sd = fmaf(ajL[f * kLd + lane], y, s * y1a);
          const float* w = w1t + (int64_t)f * oa_ld + o0;
#pragma unroll
          for (int u = 0; u < kOC; ++u) acc[u] = fmaf(w[u], sd, acc[u]);
          if (a_w1t) {
            const float e = s * y;
            const float* aw = a_w1t + (int64_t)f * oa_ld + o0;
#pragma unroll
            for (int u = 0; u < kOC; ++u) acc[u] = fmaf(aw[u], e, acc[u]);
          }
        }
      }
      if (t < T) {
#pragma unroll
        for (int u = 0; u < kOC; ++u) {
          const int o = o0 + u;
          if (o < Oa) ggS[proj_index(o, t, T, ba)] = acc[u];
        }
      }
    }
  }
}

// as triplet_proj_wgrad<false> with sdot in place of sbf: thread = feature, blockIdx.y = chunk of
// kOC output columns, triplets added in index order, one partial row per block
__global__ void triplet_proj_bwd2_wgrad(
    int64_t T, int64_t E, int n, int k, int64_t tiles_per_block, const float* __restrict__ jb,
    const float* __restrict__ a_jb, const float* __restrict__ angle,
    const float* __restrict__ a_angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ gS, int Oa, int oa_ld, int ba,
    float* __restrict__ partials) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  __shared__ float aaL[kTile];
  __shared__ float gL[kTile][kOC];
  const int nk = n * k;
  float* jbL = sm;
  float* ajL = jbL + nk * kLd;
  float* YL = ajL + nk * kLd;
  float* Y1L = YL + n * kLd;
  const int tid = threadIdx.x;
  const int o0 = blockIdx.y * kOC;
  const int f = tid;
  const bool active = f < nk;
  const int yrow = active ? f / k : 0;
  float acc[kOC];
#pragma unroll
  for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_block;
  for (int64_t tile = tile0; tile < tile0 + tiles_per_block; ++tile) {
    const int64_t t0 = tile * kTile;
    if (t0 >= T) break;
    __syncthreads();
    stage_tile2(t0, T, E, n, nk, jb, a_jb, angle, a_angle, idx_kj, pref, jbL, ajL, YL, Y1L,
                nullptr, aaL, kjL);
    for (int i = tid; i < kTile * kOC; i += blockDim.x) {
      const int r = i / kOC, u = i % kOC;
      const int o = o0 + u;
      const int64_t t = t0 + r;
      gL[r][u] = (t < T && o < Oa) ? gS[proj_index(o, t, T, ba)] : 0.f;
    }
    __syncthreads();
    if (active) {
      for (int r = 0; r < kTile; ++r) {
        const float sd = fmaf(ajL[f * kLd + r], YL[yrow * kLd + r],
                              jbL[f * kLd + r] * Y1L[yrow * kLd + r] * aaL[r]);
#pragma unroll
        for (int u = 0; u < kOC; ++u) acc[u] = fmaf(gL[r][u], sd, acc[u]);
      }
    }
  }
  if (active) {
    float* row = partials + (int64_t)blockIdx.x * nk * oa_ld;
#pragma unroll
    for (int u = 0; u < kOC; ++u) row[(int64_t)f * oa_ld + o0 + u] = acc[u];
  }
}

// as triplet_proj_geom_bwd<false>: lane = triplet; u and udot are folded chunk by chunk into the
// h_sbe row (LDS, written out coalesced) and h_angle (a register)
__global__ __launch_bounds__(kTile) void triplet_proj_bwd2_geom(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ a_jb, const float* __restrict__ angle,
    const float* __restrict__ a_angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ w1t,
    const float* __restrict__ a_w1t, int Oa, int oa_ld, int ba, const float* __restrict__ gS,
    float* __restrict__ h_jb_rows, float* __restrict__ h_angle) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  __shared__ float aaL[kTile];
  const int nk = n * k;
  float* jbL = sm;
  float* ajL = jbL + nk * kLd;
  float* hjL = ajL + nk * kLd;
  float* YL = hjL + nk * kLd;
  float* Y1L = YL + n * kLd;
  float* Y2L = Y1L + n * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile2(t0, T, E, n, nk, jb, a_jb, angle, a_angle, idx_kj, pref, jbL, ajL, YL, Y1L, Y2L,
                aaL, kjL);
    const int64_t t = t0 + lane;
    const float aa = aaL[lane];
    for (int i = 0; i < nk; ++i) hjL[i * kLd + lane] = 0.f;
    float ha = 0.f;
    for (int o0 = 0; o0 < Oa; o0 += kOC) {
      float g[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) {
        const int o = o0 + u;
        g[u] = (t < T && o < Oa) ? gS[proj_index(o, t, T, ba)] : 0.f;
      }
      for (int l = 0; l < n; ++l) {
        const float y = YL[l * kLd + lane], y1 = Y1L[l * kLd + lane];
        const float y2a = Y2L[l * kLd + lane] * aa;
        for (int q = 0; q < k; ++q) {
          const int f = l * k + q;
          const float* w = w1t + (int64_t)f * oa_ld + o0;
          float ue = 0.f, ud = 0.f;
#pragma unroll
          for (int u = 0; u < kOC; ++u) ue = fmaf(w[u], g[u], ue);
          if (a_w1t) {
            const float* aw = a_w1t + (int64_t)f * oa_ld + o0;
#pragma unroll
            for (int u = 0; u < kOC; ++u) ud = fmaf(aw[u], g[u], ud);
          }
          const float s = jbL[f * kLd + lane], as = ajL[f * kLd + lane];
          hjL[f * kLd + lane] += ud * y + ue * y1 * aa;
          ha += ud * s * y1 + ue * (as * y1 + s * y2a);
        }
      }
    }
    if (t < T) h_angle[t] = ha;
    __syncthreads();
    for (int r = 0; r < kTile && t0 + r < T; ++r)
      for (int c = lane; c < nk; c += kTile) h_jb_rows[(t0 + r) * nk + c] = hjL[c * kLd + r];
  }
}

template <bool kTorsion>
int64_t proj_bwd_blocks(int64_t T) {
  const int cap = kTorsion ? kProjBwdBlocks : kProjBwdBlocksAngleOnly;
  return std::max<int64_t>(1, std::min<int64_t>(ceil_div(T, kTile), cap));
}

unsigned tile_grid(int64_t T) {
  return (unsigned)std::min<int64_t>(ceil_div(T, kTile), (int64_t)1 << 20);
}

bool basis_ok(int n, int k) { return n >= 1 && k >= 1 && n <= 16 && k <= 64; }

// dynamic LDS of one staged tile: the jb planes and the harmonics
template <bool kTorsion>
size_t tile_lds(int n, int k) {
  return (size_t)(n * k + y_planes<kTorsion>(n)) * kLd * sizeof(float);
}

int64_t edge_basis_bwd_partial_rows(int64_t n_edges) {
  return n_edges > 0 ? ceil_div(n_edges, kEdgeT) : 0;
}

template <bool kCut>
int edge_basis_fwd_launch(const float* dist, int64_t n_edges, float cutoff, int envelope_exponent,
                          const float* freq, int num_radial, const float* zeros,
                          const float* norm, int num_spherical, float* rbf, float* jb,
                          void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0);
  if (n_edges == 0) return GMP_OK;
  GMP_CHECK_ARG(dist && freq && zeros && norm && rbf && jb);
  const int nk = num_spherical * num_radial;
  const int64_t total = n_edges * (num_radial + nk);
  GMP_CHECK_ARG(ceil_div(total, kEdgeT) <= INT32_MAX);
  edge_basis_fwd<kCut><<<(unsigned)ceil_div(total, kEdgeT), kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm, nk, rbf, jb);
  return launch_status();
}

template <bool kCut>
int edge_basis_bwd_launch(const float* dist, int64_t n_edges, float cutoff, int envelope_exponent,
                          const float* freq, int num_radial, const float* zeros,
                          const float* norm, int num_spherical, const float* grad_rbf,
                          const float* grad_jb, float* grad_dist, float* grad_freq,
                          float* freq_partials, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0 && grad_freq);
  if (n_edges == 0)
    return hip_check(hipMemsetAsync(grad_freq, 0, num_radial * sizeof(float), as_stream(stream)));
  GMP_CHECK_ARG(dist && freq && zeros && norm && grad_dist && freq_partials);
  const int64_t nb = ceil_div(n_edges, kEdgeT);
  GMP_CHECK_ARG(nb <= INT32_MAX);
  edge_basis_bwd<kCut><<<(unsigned)nb, kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm,
      num_spherical * num_radial, grad_rbf, grad_jb, grad_dist, freq_partials);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  return gmp_sum_rows_f32(freq_partials, nb, num_radial, grad_freq, stream);
}

template <bool kCut>
int edge_basis_bwd2_launch(const float* dist, int64_t n_edges, float cutoff, int envelope_exponent,
                           const float* freq, int num_radial, const float* zeros,
                           const float* norm, int num_spherical, const float* grad_rbf,
                           const float* grad_jb, const float* a_dist, const float* a_freq,
                           float* gg_rbf, float* gg_jb, float* h_dist, float* h_freq,
                           float* freq_partials, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0 && h_freq);
  if (n_edges == 0)
    return hip_check(hipMemsetAsync(h_freq, 0, num_radial * sizeof(float), as_stream(stream)));
  GMP_CHECK_ARG(dist && freq && zeros && norm && gg_rbf && gg_jb && h_dist && freq_partials);
  const int64_t nb = ceil_div(n_edges, kEdgeT);
  GMP_CHECK_ARG(nb <= INT32_MAX);
  edge_basis_bwd2<kCut><<<(unsigned)nb, kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm,
      num_spherical * num_radial, grad_rbf, grad_jb, a_dist, a_freq, gg_rbf, gg_jb, h_dist,
      freq_partials);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  return gmp_sum_rows_f32(freq_partials, nb, num_radial, h_freq, stream);
}

// The per-triplet launchers take SphereNet's argument lists; without kTorsion the torsion
// arguments (torsion, w_t1_t, bt, P and their gradients) are null / 0 and not looked at.
template <bool kTorsion>
int triplet_proj_fwd_launch(int64_t n_triplets, int64_t n_edges, int n, int k, const float* jb,
                            const float* angle, const float* torsion, const int64_t* idx_kj,
                            const float* pref, const float* w_sbf1_t, int n_layers, int ba,
                            const float* w_t1_t, int bt, float* S, float* P, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(n, k) && n_layers >= 1 && ba >= 1 &&
                (!kTorsion || bt >= 1));
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(jb && angle && idx_kj && pref && w_sbf1_t && S && n_edges > 0 &&
                (!kTorsion || (torsion && w_t1_t && P)));
  const int Oa = n_layers * ba, Ot = n_layers * bt;
  const int oa_ld = (int)ceil_div(Oa, kOC) * kOC, ot_ld = (int)ceil_div(Ot, kOC) * kOC;
  const size_t lds = tile_lds<kTorsion>(n, k);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  triplet_proj_fwd<kTorsion><<<tile_grid(n_triplets), kTile, lds, as_stream(stream)>>>(
      n_triplets, n_edges, n, k, jb, angle, idx_kj, pref, w_sbf1_t, Oa, oa_ld, ba, S, torsion,
      w_t1_t, Ot, ot_ld, bt, P);
  return launch_status();
}

template <bool kTorsion>
int triplet_emb_launch(int64_t n_triplets, int64_t n_edges, int n, int k, const float* jb,
                       const float* angle, const float* torsion, const int64_t* idx_kj,
                       const float* pref, float* angle_emb, float* torsion_emb, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(n, k));
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(jb && angle && idx_kj && pref && angle_emb && n_edges > 0 &&
                (!kTorsion || (torsion && torsion_emb)));
  const size_t lds = tile_lds<kTorsion>(n, k);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  triplet_emb<kTorsion><<<tile_grid(n_triplets), kTile, lds, as_stream(stream)>>>(
      n_triplets, n_edges, n, k, jb, angle, idx_kj, pref, angle_emb, torsion, torsion_emb);
  return launch_status();
}

template <bool kTorsion>
int triplet_proj_bwd_launch(int64_t n_triplets, int64_t n_edges, int n, int k, const float* jb,
                            const float* angle, const float* torsion, const int64_t* idx_kj,
                            const float* pref, const float* w_sbf1_t, int n_layers, int ba,
                            const float* w_t1_t, int bt, const float* grad_S, const float* grad_P,
                            float* grad_w, float* partials, float* grad_jb_rows,
                            float* grad_angle, float* grad_torsion, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(n, k) && n_layers >= 1 && ba >= 1 &&
                (!kTorsion || bt >= 1) && grad_w);
  const int nk = n * k, nnk = kTorsion ? n * nk : 0;
  const int Oa = n_layers * ba, Ot = n_layers * bt;
  const int oa_ld = (int)ceil_div(Oa, kOC) * kOC, ot_ld = (int)ceil_div(Ot, kOC) * kOC;
  const int64_t width = (int64_t)nk * oa_ld + (int64_t)nnk * ot_ld;
  hipStream_t s = as_stream(stream);
  if (n_triplets == 0) return hip_check(hipMemsetAsync(grad_w, 0, width * sizeof(float), s));
  GMP_CHECK_ARG(jb && angle && idx_kj && pref && w_sbf1_t && grad_S && partials && n_edges > 0 &&
                (!kTorsion || (torsion && w_t1_t && grad_P)));
  const int threads = (int)ceil_div(nk + nnk, kWave) * kWave;
  const size_t lds = tile_lds<kTorsion>(n, k);
  if (threads > 1024 || lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = proj_bwd_blocks<kTorsion>(n_triplets);
  const int64_t tpb = ceil_div(ceil_div(n_triplets, kTile), nb);
  const int chunks = std::max(oa_ld, ot_ld) / kOC;
  triplet_proj_wgrad<kTorsion><<<dim3((unsigned)nb, (unsigned)chunks), threads, lds, s>>>(
      n_triplets, n_edges, n, k, tpb, jb, angle, idx_kj, pref, grad_S, Oa, oa_ld, ba, partials,
      torsion, grad_P, Ot, ot_ld, bt);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  rc = gmp_sum_rows_f32(partials, nb, width, grad_w, stream);
  if (rc != GMP_OK) return rc;
  if (grad_jb_rows || grad_angle || (kTorsion && grad_torsion)) {
    GMP_CHECK_ARG(grad_jb_rows && grad_angle && (!kTorsion || grad_torsion));
    if (2 * lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
    triplet_proj_geom_bwd<kTorsion><<<tile_grid(n_triplets), kTile, 2 * lds, s>>>(
        n_triplets, n_edges, n, k, jb, angle, idx_kj, pref, w_sbf1_t, Oa, oa_ld, ba, grad_S,
        grad_jb_rows, grad_angle, torsion, w_t1_t, Ot, ot_ld, bt, grad_P, grad_torsion);
    rc = launch_status();
  }
  return rc;
}

int triplet_proj_bwd2_launch(int64_t n_triplets, int64_t n_edges, int n, int k, const float* jb,
                             const float* angle, const int64_t* idx_kj, const float* pref,
                             const float* w_sbf1_t, int n_layers, int ba, const float* grad_S,
                             const float* a_jb, const float* a_angle, const float* a_w_t,
                             float* gg_S, float* h_w, float* partials, float* h_jb_rows,
                             float* h_angle, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(n, k) && n_layers >= 1 && ba >= 1 &&
                h_w);
  const int nk = n * k;
  const int Oa = n_layers * ba;
  const int oa_ld = (int)ceil_div(Oa, kOC) * kOC;
  const int64_t width = (int64_t)nk * oa_ld;
  hipStream_t s = as_stream(stream);
  if (n_triplets == 0) return hip_check(hipMemsetAsync(h_w, 0, width * sizeof(float), s));
  GMP_CHECK_ARG(jb && angle && idx_kj && pref && w_sbf1_t && grad_S && gg_S && partials &&
                n_edges > 0 && (!h_jb_rows == !h_angle));
  const int threads = (int)ceil_div(nk, kWave) * kWave;
  const size_t lds2 = (size_t)(2 * nk + 2 * n) * kLd * sizeof(float);
  const size_t lds3 = (size_t)(3 * nk + 3 * n) * kLd * sizeof(float);
  if (threads > 1024 || lds2 > kLdsCap || (h_angle && lds3 > kLdsCap)) return GMP_ERR_UNSUPPORTED;
  triplet_proj_bwd2_ggs<<<tile_grid(n_triplets), kTile, lds2, s>>>(
      n_triplets, n_edges, n, k, jb, a_jb, angle, a_angle, idx_kj, pref, w_sbf1_t, a_w_t, Oa,
      oa_ld, ba, gg_S);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  const int64_t nb = proj_bwd_blocks<false>(n_triplets);
  const int64_t tpb = ceil_div(ceil_div(n_triplets, kTile), nb);
  triplet_proj_bwd2_wgrad<<<dim3((unsigned)nb, (unsigned)(oa_ld / kOC)), threads, lds2, s>>>(
      n_triplets, n_edges, n, k, tpb, jb, a_jb, angle, a_angle, idx_kj, pref, grad_S, Oa, oa_ld,
      ba, partials);
  rc = launch_status();
  if (rc != GMP_OK) return rc;
  rc = gmp_sum_rows_f32(partials, nb, width, h_w, stream);
  if (rc != GMP_OK) return rc;
  if (h_angle) {
    triplet_proj_bwd2_geom<<<tile_grid(n_triplets), kTile, lds3, s>>>(
        n_triplets, n_edges, n, k, jb, a_jb, angle, a_angle, idx_kj, pref, w_sbf1_t, a_w_t, Oa,
        oa_ld, ba, grad_S, h_jb_rows, h_angle);
    rc = launch_status();
  }
  return rc;
}

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int64_t gmp_sph_edge_basis_bwd_partial_rows(int64_t n_edges) {
  return edge_basis_bwd_partial_rows(n_edges);
}

int64_t gmp_dime_edge_basis_bwd_partial_rows(int64_t n_edges) {
  return edge_basis_bwd_partial_rows(n_edges);
}

int gmp_sph_edge_basis_fwd_f32(const float* dist, int64_t n_edges, float cutoff,
                               int envelope_exponent, const float* freq, int num_radial,
                               const float* zeros, const float* norm, int num_spherical,
                               float* rbf, float* jb, void* stream) {
  return edge_basis_fwd_launch<false>(dist, n_edges, cutoff, envelope_exponent, freq, num_radial,
                                      zeros, norm, num_spherical, rbf, jb, stream);
}

int gmp_dime_edge_basis_fwd_f32(const float* dist, int64_t n_edges, float cutoff,
                                int envelope_exponent, const float* freq, int num_radial,
                                const float* zeros, const float* norm, int num_spherical,
                                float* rbf, float* sbe, void* stream) {
  return edge_basis_fwd_launch<true>(dist, n_edges, cutoff, envelope_exponent, freq, num_radial,
                                     zeros, norm, num_spherical, rbf, sbe, stream);
}

int gmp_sph_edge_basis_bwd_f32(const float* dist, int64_t n_edges, float cutoff,
                               int envelope_exponent, const float* freq, int num_radial,
                               const float* zeros, const float* norm, int num_spherical,
                               const float* grad_rbf, const float* grad_jb, float* grad_dist,
                               float* grad_freq, float* freq_partials, void* stream) {
  return edge_basis_bwd_launch<false>(dist, n_edges, cutoff, envelope_exponent, freq, num_radial,
                                      zeros, norm, num_spherical, grad_rbf, grad_jb, grad_dist,
                                      grad_freq, freq_partials, stream);
}

int gmp_dime_edge_basis_bwd_f32(const float* dist, int64_t n_edges, float cutoff,
                                int envelope_exponent, const float* freq, int num_radial,
                                const float* zeros, const float* norm, int num_spherical,
                                const float* grad_rbf, const float* grad_sbe, float* grad_dist,
                                float* grad_freq, float* freq_partials, void* stream) {
  return edge_basis_bwd_launch<true>(dist, n_edges, cutoff, envelope_exponent, freq, num_radial,
                                     zeros, norm, num_spherical, grad_rbf, grad_sbe, grad_dist,
                                     grad_freq, freq_partials, stream);
}

int64_t gmp_dime_edge_basis_bwd2_partial_rows(int64_t n_edges) {
  return edge_basis_bwd_partial_rows(n_edges);
}

int gmp_dime_edge_basis_bwd2_f32(const float* dist, int64_t n_edges, float cutoff,
                                 int envelope_exponent, const float* freq, int num_radial,
                                 const float* zeros, const float* norm, int num_spherical,
                                 const float* grad_rbf, const float* grad_sbe,
                                 const float* a_dist, const float* a_freq, float* gg_rbf,
                                 float* gg_sbe, float* h_dist, float* h_freq,
                                 float* freq_partials, void* stream) {
  return edge_basis_bwd2_launch<true>(dist, n_edges, cutoff, envelope_exponent, freq, num_radial,
                                      zeros, norm, num_spherical, grad_rbf, grad_sbe, a_dist,
                                      a_freq, gg_rbf, gg_sbe, h_dist, h_freq, freq_partials,
                                      stream);
}

int gmp_sph_triplet_proj_fwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                 int num_radial, const float* jb, const float* angle,
                                 const float* torsion, const int64_t* idx_kj, const float* pref,
                                 const float* w_sbf1_t, int n_layers, int ba, const float* w_t1_t,
                                 int bt, float* S, float* P, void* stream) {
  return triplet_proj_fwd_launch<true>(n_triplets, n_edges, num_spherical, num_radial, jb, angle,
                                       torsion, idx_kj, pref, w_sbf1_t, n_layers, ba, w_t1_t, bt,
                                       S, P, stream);
}

int gmp_dime_triplet_proj_fwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                  int num_radial, const float* sbe, const float* angle,
                                  const int64_t* idx_kj, const float* pref, const float* w_sbf1_t,
                                  int n_layers, int b, float* S, void* stream) {
  return triplet_proj_fwd_launch<false>(n_triplets, n_edges, num_spherical, num_radial, sbe, angle,
                                        nullptr, idx_kj, pref, w_sbf1_t, n_layers, b, nullptr, 0,
                                        S, nullptr, stream);
}

int gmp_sph_triplet_emb_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                            int num_radial, const float* jb, const float* angle,
                            const float* torsion, const int64_t* idx_kj, const float* pref,
                            float* angle_emb, float* torsion_emb, void* stream) {
  return triplet_emb_launch<true>(n_triplets, n_edges, num_spherical, num_radial, jb, angle,
                                  torsion, idx_kj, pref, angle_emb, torsion_emb, stream);
}

int gmp_dime_triplet_emb_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                             int num_radial, const float* sbe, const float* angle,
                             const int64_t* idx_kj, const float* pref, float* sbf, void* stream) {
  return triplet_emb_launch<false>(n_triplets, n_edges, num_spherical, num_radial, sbe, angle,
                                   nullptr, idx_kj, pref, sbf, nullptr, stream);
}

int64_t gmp_sph_triplet_proj_bwd_partial_rows(int64_t n_triplets) {
  return proj_bwd_blocks<true>(n_triplets);
}

int64_t gmp_dime_triplet_proj_bwd_partial_rows(int64_t n_triplets) {
  return proj_bwd_blocks<false>(n_triplets);
}

int gmp_sph_triplet_proj_bwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                 int num_radial, const float* jb, const float* angle,
                                 const float* torsion, const int64_t* idx_kj, const float* pref,
                                 const float* w_sbf1_t, int n_layers, int ba, const float* w_t1_t,
                                 int bt, const float* grad_S, const float* grad_P,
                                 float* grad_w, float* partials, float* grad_jb_rows,
                                 float* grad_angle, float* grad_torsion, void* stream) {
  return triplet_proj_bwd_launch<true>(n_triplets, n_edges, num_spherical, num_radial, jb, angle,
                                       torsion, idx_kj, pref, w_sbf1_t, n_layers, ba, w_t1_t, bt,
                                       grad_S, grad_P, grad_w, partials, grad_jb_rows, grad_angle,
                                       grad_torsion, stream);
}

int gmp_dime_triplet_proj_bwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                  int num_radial, const float* sbe, const float* angle,
                                  const int64_t* idx_kj, const float* pref, const float* w_sbf1_t,
                                  int n_layers, int b, const float* grad_S, float* grad_w,
                                  float* partials, float* grad_sbe_rows, float* grad_angle,
                                  void* stream) {
  return triplet_proj_bwd_launch<false>(n_triplets, n_edges, num_spherical, num_radial, sbe, angle,
                                        nullptr, idx_kj, pref, w_sbf1_t, n_layers, b, nullptr, 0,
                                        grad_S, nullptr, grad_w, partials, grad_sbe_rows,
                                        grad_angle, nullptr, stream);
}

int64_t gmp_dime_triplet_proj_bwd2_partial_rows(int64_t n_triplets) {
  return proj_bwd_blocks<false>(n_triplets);
}

int gmp_dime_triplet_proj_bwd2_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                   int num_radial, const float* sbe, const float* angle,
                                   const int64_t* idx_kj, const float* pref,
                                   const float* w_sbf1_t, int n_layers, int b,
                                   const float* grad_S, const float* a_sbe, const float* a_angle,
                                   const float* a_w_t, float* gg_S, float* h_w, float* partials,
                                   float* h_sbe_rows, float* h_angle, void* stream) {
  return triplet_proj_bwd2_launch(n_triplets, n_edges, num_spherical, num_radial, sbe, angle,
                                  idx_kj, pref, w_sbf1_t, n_layers, b, grad_S, a_sbe, a_angle,
                                  a_w_t, gg_S, h_w, partials, h_sbe_rows, h_angle, stream);
}

}  // extern "C"
