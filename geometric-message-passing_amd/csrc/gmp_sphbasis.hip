// K18: SphereNet's spherical basis (models/layers/spherenet_layer.py: dist_emb, angle_emb,
// torsion_emb) without the per-triplet embeddings in HBM.
//
// Per edge (gmp_sph_edge_basis_*): rbf[q] = envelope(x) sin(freq_q x) and jb[l, q] =
// N_lq j_l(z_lq x), x = d / cutoff.  The reference evaluates j_l by its closed form
// (sin / cos over powers of x), which cancels catastrophically for small arguments: j_6 at
// x = 0.05 comes out as -0.6 in fp32 where the value is ~1e-9.  Here j_l is a power series
// below x = l + 1 (all terms after the first few decrease, no cancellation) and the upward
// recurrence from j_0, j_1 above (stable for x > l).  E is small next to T, so the per-edge
// arithmetic runs in double and is rounded once.
//
// Per triplet (gmp_sph_triplet_proj_*): the n k angle features jb[kj][l, q] Y_l0(theta) and the
// n^2 k torsion features jb[kj][b, q] Yflat[a n + b](theta, phi) are formed in LDS from the
// gathered jb row and the n^2 real harmonics of the triplet, and multiplied at once into the
// first projections of every layer: S (L, T, ba), P (L, T, bt).  The reference's layout is kept:
// per l the harmonics are ordered m = 0, 1..l (cos), -l..-1 (sin), and the view(-1, n, n, 1)
// of torsion_emb pairs Bessel order b with flat harmonic a n + b.
#include <algorithm>

#include "gmp_common.h"

namespace gmp {
namespace {

constexpr int kTile = 64;        // triplets per tile (one per lane)
constexpr int kLd = kTile + 1;   // LDS row stride of the staged [feature][triplet] planes
constexpr int kOC = 8;           // output columns per accumulator chunk
constexpr int kProjBwdBlocks = 512;
constexpr int kEdgeT = 256;

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

struct Env {
  double a, b, c;
  int p;
};
__device__ Env make_env(int exponent) {
  Env e;
  e.p = exponent + 1;
  e.a = -(double)(e.p + 1) * (e.p + 2) / 2.0;
  e.b = (double)e.p * (e.p + 2);
  e.c = -(double)e.p * (e.p + 1) / 2.0;
  return e;
}
__device__ double ipow(double x, int n) {
  double r = 1.0;
  for (int i = 0; i < n; ++i) r *= x;
  return r;
}
// envelope(x) = 1/x + a x^(p-1) + b x^p + c x^(p+1) and its derivative
__device__ void env_eval(const Env& e, double x, double* v, double* dv) {
  const double x0 = ipow(x, e.p - 1);
  const double x1 = x0 * x, x2 = x1 * x;
  *v = 1.0 / x + e.a * x0 + e.b * x1 + e.c * x2;
  const double xm = e.p >= 2 ? ipow(x, e.p - 2) : 0.0;
  *dv = -1.0 / (x * x) + e.a * (double)(e.p - 1) * xm + e.b * (double)e.p * x0 +
        e.c * (double)(e.p + 1) * x1;
}

// thread per (edge, column), columns [0, k) = rbf, [k, k + n k) = jb
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
  if (c < k) {
    double v, dv;
    env_eval(make_env(exponent), x, &v, &dv);
    rbf[e * k + c] = (float)(v * sin((double)freq[c] * x));
  } else {
    const int lq = c - k;
    jb[e * nk + lq] = (float)((double)norm[lq] * sph_jl(lq / k, (double)zeros[lq] * x));
  }
}

// thread per edge: g_dist[e]; the freq gradient of the block's edges is tree-summed in LDS in
// a fixed order into one partial row per block.
__global__ __launch_bounds__(kEdgeT) void edge_basis_bwd(
    const float* __restrict__ dist, int64_t E, float cutoff, int exponent,
    const float* __restrict__ freq, int k, const float* __restrict__ zeros,
    const float* __restrict__ norm, int nk, const float* __restrict__ g_rbf,
    const float* __restrict__ g_jb, float* __restrict__ g_dist,
    float* __restrict__ freq_partials) {
  __shared__ float red[kEdgeT];
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool live = e < E;
  const double x = live ? (double)dist[e] / (double)cutoff : 1.0;
  const double inv_c = 1.0 / (double)cutoff;
  double env = 0.0, denv = 0.0;
  env_eval(make_env(exponent), x, &env, &denv);
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
  if (!live) return;
  if (g_jb) {
    for (int lq = 0; lq < nk; ++lq) {
      const double z = (double)zeros[lq];
      gd += (double)g_jb[e * nk + lq] * (double)norm[lq] * z * inv_c * sph_jl_prime(lq / k, z * x);
    }
  }
  g_dist[e] = (float)gd;
}

// The n^2 real harmonics of one direction, flat index l^2 + p with p = 0 (m = 0), 1..l (cos m
// = p), l + 1..2l (sin m = 2l + 1 - p).  Y_l^m = pref[l^2 + p] P_l^m(cos theta) {C_m, S_m} with
// C_m + i S_m = (sin theta e^{i phi})^m and P_l^m the polynomial part of the associated
// Legendre function (the sin^m theta factor lives in C_m, S_m), built by the recurrences of
// the reference's generator; pref carries the sqrt(2) of m != 0.
// kGrad: instead of storing Y, returns sum_idx gY[idx] dY[idx]/dtheta and /dphi.
template <bool kGrad>
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
  for (int m = 0; m < n; ++m) {
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
        if (kGrad) gt += Y[base * stride] * f * dp * (-st);
        else Y[base * stride] = f * p;
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
      sph_harmonics<false>(n, angle[t0 + tid], torsion[t0 + tid], pref, YL + tid, kLd, nullptr,
                           nullptr);
    } else {
      for (int i = 0; i < n * n; ++i) YL[i * kLd + tid] = 0.f;
    }
  }
  __syncthreads();
}

// one wave per tile, lane = triplet.  w1t (n k, oa_ld), w2t (n^2 k, ot_ld): feature-major,
// columns o = layer * b + j, leading dimensions padded to a multiple of kOC with zeros.
__global__ __launch_bounds__(kTile) void triplet_proj_fwd(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ angle,
    const float* __restrict__ torsion, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ w1t, int Oa, int oa_ld, int ba,
    const float* __restrict__ w2t, int Ot, int ot_ld, int bt, float* __restrict__ S,
    float* __restrict__ P) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k, nn = n * n;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    const int64_t t = t0 + lane;
    for (int o0 = 0; o0 < Oa; o0 += kOC) {
      float acc[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
      for (int l = 0; l < n; ++l) {
        const float y = YL[l * l * kLd + lane];
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
          if (o < Oa) S[((int64_t)(o / ba) * T + t) * ba + o % ba] = acc[u];
        }
      }
    }
    for (int o0 = 0; o0 < Ot; o0 += kOC) {
      float acc[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
      for (int ab = 0; ab < nn; ++ab) {
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
          if (o < Ot) P[((int64_t)(o / bt) * T + t) * bt + o % bt] = acc[u];
        }
      }
    }
  }
}

// the materialising form: angle_emb (T, n k), torsion_emb (T, n^2 k)
__global__ __launch_bounds__(kTile) void triplet_emb(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ angle,
    const float* __restrict__ torsion, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, float* __restrict__ aemb, float* __restrict__ temb) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k, nnk = n * n * k;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    for (int r = 0; r < kTile && t0 + r < T; ++r) {
      for (int f = lane; f < nk; f += kTile) {
        const int l = f / k;
        aemb[(t0 + r) * nk + f] = jbL[f * kLd + r] * YL[l * l * kLd + r];
      }
      for (int f = lane; f < nnk; f += kTile) {
        const int ab = f / k, q = f - ab * k;
        temb[(t0 + r) * nnk + f] = jbL[((ab % n) * k + q) * kLd + r] * YL[ab * kLd + r];
      }
    }
  }
}

// Weight gradients: block b sums its contiguous range of tiles, thread = feature (angle
// features first, then torsion features), blockIdx.y = chunk of kOC output columns; triplets
// are added in index order.  One partial row [g_w1t | g_w2t] per block.
__global__ void triplet_proj_wgrad(
    int64_t T, int64_t E, int n, int k, int64_t tiles_per_block, const float* __restrict__ jb,
    const float* __restrict__ angle, const float* __restrict__ torsion,
    const int64_t* __restrict__ idx_kj, const float* __restrict__ pref,
    const float* __restrict__ gS, int Oa, int oa_ld, int ba, const float* __restrict__ gP, int Ot,
    int ot_ld, int bt, float* __restrict__ partials) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  __shared__ float gL[2][kTile][kOC];
  const int nk = n * k, nnk = n * n * k;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  const int tid = threadIdx.x;
  const int o0 = blockIdx.y * kOC;
  const int f = tid;
  const bool is_a = f < nk, is_t = f >= nk && f < nk + nnk;
  int jrow = 0, yrow = 0;
  if (is_a) {
    jrow = f, yrow = (f / k) * (f / k);
  } else if (is_t) {
    const int ft = f - nk, ab = ft / k;
    jrow = (ab % n) * k + (ft - ab * k), yrow = ab;
  }
  const int which = is_a ? 0 : 1;
  const bool active = (is_a && o0 < Oa) || (is_t && o0 < Ot);
  float acc[kOC];
#pragma unroll
  for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_block;
  for (int64_t tile = tile0; tile < tile0 + tiles_per_block; ++tile) {
    const int64_t t0 = tile * kTile;
    if (t0 >= T) break;
    __syncthreads();
    stage_tile(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    for (int i = tid; i < 2 * kTile * kOC; i += blockDim.x) {
      const int w = i / (kTile * kOC), r = (i / kOC) % kTile, u = i % kOC;
      const int o = o0 + u;
      const int64_t t = t0 + r;
      float v = 0.f;
      if (t < T) {
        if (w == 0 && o < Oa) v = gS[((int64_t)(o / ba) * T + t) * ba + o % ba];
        if (w == 1 && o < Ot) v = gP[((int64_t)(o / bt) * T + t) * bt + o % bt];
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
  if (is_a && o0 < oa_ld) {
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
// the harmonics' derivatives turn into g_angle and g_torsion.
__global__ __launch_bounds__(kTile) void triplet_proj_geom_bwd(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ jb,
    const float* __restrict__ angle,
    const float* __restrict__ torsion, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ w1t, int Oa, int oa_ld, int ba,
    const float* __restrict__ w2t, int Ot, int ot_ld, int bt, const float* __restrict__ gS,
    const float* __restrict__ gP, float* __restrict__ g_jb_rows, float* __restrict__ g_angle,
    float* __restrict__ g_torsion) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k, nn = n * n;
  float* jbL = sm;
  float* YL = sm + nk * kLd;
  float* gjL = YL + nn * kLd;
  float* gyL = gjL + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    stage_tile(t0, T, E, n, nk, jb, angle, torsion, idx_kj, pref, jbL, YL, kjL);
    const int64_t t = t0 + lane;
    for (int i = 0; i < nk; ++i) gjL[i * kLd + lane] = 0.f;
    for (int i = 0; i < nn; ++i) gyL[i * kLd + lane] = 0.f;
    for (int o0 = 0; o0 < Oa; o0 += kOC) {
      float g[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) {
        const int o = o0 + u;
        g[u] = (t < T && o < Oa) ? gS[((int64_t)(o / ba) * T + t) * ba + o % ba] : 0.f;
      }
      for (int l = 0; l < n; ++l) {
        const float y = YL[l * l * kLd + lane];
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
        gyL[l * l * kLd + lane] += gy;
      }
    }
    for (int o0 = 0; o0 < Ot; o0 += kOC) {
      float g[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) {
        const int o = o0 + u;
        g[u] = (t < T && o < Ot) ? gP[((int64_t)(o / bt) * T + t) * bt + o % bt] : 0.f;
      }
      for (int ab = 0; ab < nn; ++ab) {
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
    if (t < T) {
      float gt, gp;
      sph_harmonics<true>(n, angle[t], torsion[t], pref, gyL + lane, kLd, &gt, &gp);
      g_angle[t] = gt;
      g_torsion[t] = gp;
    }
    __syncthreads();
    for (int r = 0; r < kTile && t0 + r < T; ++r)
      for (int c = lane; c < nk; c += kTile) g_jb_rows[(t0 + r) * nk + c] = gjL[c * kLd + r];
  }
}

int64_t proj_bwd_blocks(int64_t T) {
  return std::max<int64_t>(1, std::min<int64_t>(ceil_div(T, kTile), kProjBwdBlocks));
}

unsigned tile_grid(int64_t T) {
  return (unsigned)std::min<int64_t>(ceil_div(T, kTile), (int64_t)1 << 20);
}

bool basis_ok(int n, int k) { return n >= 1 && k >= 1 && n <= 16 && k <= 64; }

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int64_t gmp_sph_edge_basis_bwd_partial_rows(int64_t n_edges) {
  return n_edges > 0 ? ceil_div(n_edges, kEdgeT) : 0;
}

int gmp_sph_edge_basis_fwd_f32(const float* dist, int64_t n_edges, float cutoff,
                               int envelope_exponent, const float* freq, int num_radial,
                               const float* zeros, const float* norm, int num_spherical,
                               float* rbf, float* jb, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0);
  if (n_edges == 0) return GMP_OK;
  GMP_CHECK_ARG(dist && freq && zeros && norm && rbf && jb);
  const int nk = num_spherical * num_radial;
  const int64_t total = n_edges * (num_radial + nk);
  GMP_CHECK_ARG(ceil_div(total, kEdgeT) <= INT32_MAX);
  edge_basis_fwd<<<(unsigned)ceil_div(total, kEdgeT), kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm, nk, rbf, jb);
  return launch_status();
}

int gmp_sph_edge_basis_bwd_f32(const float* dist, int64_t n_edges, float cutoff,
                               int envelope_exponent, const float* freq, int num_radial,
                               const float* zeros, const float* norm, int num_spherical,
                               const float* grad_rbf, const float* grad_jb, float* grad_dist,
                               float* grad_freq, float* freq_partials, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0 && grad_freq);
  if (n_edges == 0)
    return hip_check(hipMemsetAsync(grad_freq, 0, num_radial * sizeof(float), as_stream(stream)));
  GMP_CHECK_ARG(dist && freq && zeros && norm && grad_dist && freq_partials);
  const int64_t nb = ceil_div(n_edges, kEdgeT);
  GMP_CHECK_ARG(nb <= INT32_MAX);
  edge_basis_bwd<<<(unsigned)nb, kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm,
      num_spherical * num_radial, grad_rbf, grad_jb, grad_dist, freq_partials);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  return gmp_sum_rows_f32(freq_partials, nb, num_radial, grad_freq, stream);
}

int gmp_sph_triplet_proj_fwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                 int num_radial, const float* jb, const float* angle,
                                 const float* torsion, const int64_t* idx_kj, const float* pref,
                                 const float* w_sbf1_t, int n_layers, int ba, const float* w_t1_t,
                                 int bt, float* S, float* P, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(num_spherical, num_radial) &&
                n_layers >= 1 && ba >= 1 && bt >= 1);
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(jb && angle && torsion && idx_kj && pref && w_sbf1_t && w_t1_t && S && P &&
                n_edges > 0);
  const int Oa = n_layers * ba, Ot = n_layers * bt;
  const int oa_ld = (int)ceil_div(Oa, kOC) * kOC, ot_ld = (int)ceil_div(Ot, kOC) * kOC;
  const size_t lds = (size_t)(num_spherical * num_radial + num_spherical * num_spherical) * kLd *
                     sizeof(float);
  if (lds > 60 * 1024) return GMP_ERR_UNSUPPORTED;
  triplet_proj_fwd<<<tile_grid(n_triplets), kTile, lds, as_stream(stream)>>>(
      n_triplets, n_edges, num_spherical, num_radial, jb, angle, torsion, idx_kj, pref, w_sbf1_t,
      Oa,
      oa_ld, ba, w_t1_t, Ot, ot_ld, bt, S, P);
  return launch_status();
}

int gmp_sph_triplet_emb_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                            int num_radial, const float* jb, const float* angle,
                            const float* torsion, const int64_t* idx_kj, const float* pref,
                            float* angle_emb, float* torsion_emb, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(num_spherical, num_radial));
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(jb && angle && torsion && idx_kj && pref && angle_emb && torsion_emb &&
                n_edges > 0);
  const size_t lds = (size_t)(num_spherical * num_radial + num_spherical * num_spherical) * kLd *
                     sizeof(float);
  if (lds > 60 * 1024) return GMP_ERR_UNSUPPORTED;
  triplet_emb<<<tile_grid(n_triplets), kTile, lds, as_stream(stream)>>>(
      n_triplets, n_edges, num_spherical, num_radial, jb, angle, torsion, idx_kj, pref, angle_emb,
      torsion_emb);
  return launch_status();
}

int64_t gmp_sph_triplet_proj_bwd_partial_rows(int64_t n_triplets) {
  return proj_bwd_blocks(n_triplets);
}

int gmp_sph_triplet_proj_bwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                 int num_radial, const float* jb, const float* angle,
                                 const float* torsion, const int64_t* idx_kj, const float* pref,
                                 const float* w_sbf1_t, int n_layers, int ba, const float* w_t1_t,
                                 int bt, const float* grad_S, const float* grad_P,
                                 float* grad_w, float* partials, float* grad_jb_rows,
                                 float* grad_angle, float* grad_torsion, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(num_spherical, num_radial) &&
                n_layers >= 1 && ba >= 1 && bt >= 1 && grad_w);
  const int n = num_spherical, k = num_radial, nk = n * k, nnk = n * n * k;
  const int Oa = n_layers * ba, Ot = n_layers * bt;
  const int oa_ld = (int)ceil_div(Oa, kOC) * kOC, ot_ld = (int)ceil_div(Ot, kOC) * kOC;
  const int64_t width = (int64_t)nk * oa_ld + (int64_t)nnk * ot_ld;
  hipStream_t s = as_stream(stream);
  if (n_triplets == 0) return hip_check(hipMemsetAsync(grad_w, 0, width * sizeof(float), s));
  GMP_CHECK_ARG(jb && angle && torsion && idx_kj && pref && w_sbf1_t && w_t1_t && grad_S &&
                grad_P && partials && n_edges > 0);
  const int feats = nk + nnk;
  const int threads = (int)ceil_div(feats, kWave) * kWave;
  const size_t lds = (size_t)(nk + n * n) * kLd * sizeof(float);
  if (threads > 1024 || lds > 60 * 1024) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = proj_bwd_blocks(n_triplets);
  const int64_t tpb = ceil_div(ceil_div(n_triplets, kTile), nb);
  const int chunks = std::max(oa_ld, ot_ld) / kOC;
  triplet_proj_wgrad<<<dim3((unsigned)nb, (unsigned)chunks), threads, lds, s>>>(
      n_triplets, n_edges, n, k, tpb, jb, angle, torsion, idx_kj, pref, grad_S, Oa, oa_ld, ba,
      grad_P, Ot, ot_ld, bt, partials);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  rc = gmp_sum_rows_f32(partials, nb, width, grad_w, stream);
  if (rc != GMP_OK) return rc;
  if (grad_jb_rows || grad_angle || grad_torsion) {
    GMP_CHECK_ARG(grad_jb_rows && grad_angle && grad_torsion);
    if (2 * lds > 60 * 1024) return GMP_ERR_UNSUPPORTED;
    triplet_proj_geom_bwd<<<tile_grid(n_triplets), kTile, 2 * lds, s>>>(
        n_triplets, n_edges, n, k, jb, angle, torsion, idx_kj, pref, w_sbf1_t, Oa, oa_ld, ba,
        w_t1_t, Ot, ot_ld, bt, grad_S, grad_P, grad_jb_rows, grad_angle, grad_torsion);
    rc = launch_status();
  }
  return rc;
}

}  // extern "C"
