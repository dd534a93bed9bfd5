// K18d / K19d: DimeNet++'s angle-only spherical basis and triplet interaction (PyG 2.3.1
// DimeNetPlusPlus: BesselBasisLayer, SphericalBasisLayer, InteractionPPBlock), the forms of K18 /
// K19 (gmp_sphbasis.hip, gmp_tripletmp.hip) without the torsion factor:
//
//   rbf[e, q]         = env(x) sin(freq_q x),            env(x) = envelope(x) [x < 1], x = d / cutoff
//   sbe[e, l k + q]   = env(x) N_lq j_l(z_lq x)
//   sbf[t, l k + q]   = sbe[idx_kj[t], l k + q] Y_l0(angle_t)      (never written by the model)
//   S[layer, t, :]    = W_sbf1[layer] sbf_t
//   m[e, c]           = sum_{t of e} xd[idx_kj[t], c] (W_sbf2 S_t)[c]
//
// Only the n Legendre values of a triplet are formed (K18 forms the n^2 harmonics), and K19d's
// gradient kernel keeps its weight-gradient accumulators in registers (lane = channel) and reduces
// the b per-triplet sums of grad_S with one transposing butterfly.  The device helpers shared with
// K18 (j_l, the envelope) are copies: the objects of the SphereNet kernels stay as they were.
#include <algorithm>

#include "gmp_common.h"

namespace gmp {
namespace {

constexpr int kTile = 64;        // triplets per tile (one per lane)
constexpr int kLd = kTile + 1;   // LDS row stride of the staged [feature][triplet] planes
constexpr int kOC = 8;           // output columns per accumulator chunk
// The weight-gradient blocks are one wave at the default basis (n k = 42 features <= 64), so the
// grid is what fills the chip: 4096 blocks (0.69 ms at 3.5M triplets; 2.29 ms at K18's cap, 512).
constexpr int kProjBwdBlocks = 4096;
constexpr int kEdgeT = 256;
constexpr int kWaves = 4;        // waves per block of K19d
constexpr int kMaxB = 16;        // basis_emb_size <= kMaxB in K19d's backward
constexpr int kBwdBlocks = 2048;
constexpr size_t kLdsCap = 60 * 1024;

// j_l(x) for x > 0: the series below x = l + 1, the upward recurrence above (as K18)
__device__ double dime_jl(int l, double x) {
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
__device__ double dime_jl_prime(int l, double x) {
  if (l == 0) return -dime_jl(1, x);
  return dime_jl(l - 1, x) - (double)(l + 1) / x * dime_jl(l, x);
}

__device__ double dime_ipow(double x, int n) {
  double r = 1.0;
  for (int i = 0; i < n; ++i) r *= x;
  return r;
}

// envelope(x) = 1/x + a x^(p-1) + b x^p + c x^(p+1) and its derivative, 0 < x < 1
__device__ void dime_env(int exponent, double x, double* v, double* dv) {
  const int p = exponent + 1;
  const double a = -(double)(p + 1) * (p + 2) / 2.0, b = (double)p * (p + 2),
               c = -(double)p * (p + 1) / 2.0;
  const double x0 = dime_ipow(x, p - 1);
  const double x1 = x0 * x, x2 = x1 * x;
  *v = 1.0 / x + a * x0 + b * x1 + c * x2;
  const double xm = p >= 2 ? dime_ipow(x, p - 2) : 0.0;
  *dv = -1.0 / (x * x) + a * (double)(p - 1) * xm + b * (double)p * x0 + c * (double)(p + 1) * x1;
}

// thread per (edge, column), columns [0, k) = rbf, [k, k + n k) = sbe; zero at and past the cutoff
__global__ __launch_bounds__(kEdgeT) void dime_edge_basis_fwd(
    const float* __restrict__ dist, int64_t E, float cutoff, int exponent,
    const float* __restrict__ freq, int k, const float* __restrict__ zeros,
    const float* __restrict__ norm, int nk, float* __restrict__ rbf, float* __restrict__ sbe) {
  const int cols = k + nk;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= E * cols) return;
  const int64_t e = i / cols;
  const int c = (int)(i - e * cols);
  const double x = (double)dist[e] / (double)cutoff;
  float out = 0.f;
  if (x < 1.0) {
    double v, dv;
    dime_env(exponent, x, &v, &dv);
    if (c < k) {
      out = (float)(v * sin((double)freq[c] * x));
    } else {
      const int lq = c - k;
      out = (float)(v * (double)norm[lq] * dime_jl(lq / k, (double)zeros[lq] * x));
    }
  }
  if (c < k) rbf[e * k + c] = out;
  else sbe[e * nk + (c - k)] = out;
}

// thread per edge: g_dist[e]; the freq gradient of the block's edges is tree-summed in LDS in
// a fixed order into one partial row per block.
__global__ __launch_bounds__(kEdgeT) void dime_edge_basis_bwd(
    const float* __restrict__ dist, int64_t E, float cutoff, int exponent,
    const float* __restrict__ freq, int k, const float* __restrict__ zeros,
    const float* __restrict__ norm, int nk, const float* __restrict__ g_rbf,
    const float* __restrict__ g_sbe, float* __restrict__ g_dist,
    float* __restrict__ freq_partials) {
  __shared__ float red[kEdgeT];
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool in_range = e < E;
  const double xr = in_range ? (double)dist[e] / (double)cutoff : 1.0;
  const bool live = in_range && xr < 1.0;
  const double x = live ? xr : 0.5;
  const double inv_c = 1.0 / (double)cutoff;
  double env = 0.0, denv = 0.0;
  dime_env(exponent, x, &env, &denv);
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
  if (live && g_sbe) {
    for (int lq = 0; lq < nk; ++lq) {
      const double z = (double)zeros[lq];
      const int l = lq / k;
      gd += (double)g_sbe[e * nk + lq] * (double)norm[lq] * inv_c *
            (denv * dime_jl(l, z * x) + env * z * dime_jl_prime(l, z * x));
    }
  }
  g_dist[e] = live ? (float)gd : 0.f;
}

// Y_l0(theta) = pref[l^2] P_l(cos theta), l < n, by the Legendre recurrence (the m = 0 branch of
// K18's harmonics).  kGrad: instead of storing Y, returns sum_l gY[l] dY_l0/dtheta.
template <bool kGrad>
__device__ float legendre_m0(int n, float theta, const float* __restrict__ pref, float* Y,
                             int stride) {
  float st, ct;
  sincosf(theta, &st, &ct);
  float p2 = 0.f, dp2 = 0.f, p1 = 0.f, dp1 = 0.f, gt = 0.f;
  for (int l = 0; l < n; ++l) {
    float p, dp;
    if (l == 0) {
      p = 1.f, dp = 0.f;
    } else if (l == 1) {
      p = ct * p1, dp = p1;
    } else {
      const float inv = 1.f / (float)l;
      p = ((float)(2 * l - 1) * ct * p1 - (float)(l - 1) * p2) * inv;
      dp = ((float)(2 * l - 1) * (p1 + ct * dp1) - (float)(l - 1) * dp2) * inv;
    }
    p2 = p1, dp2 = dp1, p1 = p, dp1 = dp;
    const float f = pref[l * l];
    if (kGrad) gt += Y[l * stride] * f * dp * (-st);
    else Y[l * stride] = f * p;
  }
  return gt;
}

// Stage one tile: sbL[c * kLd + r] = sbe[idx_kj[t0 + r], c] (coalesced rows), YL[l * kLd + r] =
// Y_l0(angle[t0 + r]).  kjL (kTile ints) is scratch.  All threads of the block take part; ends
// with a barrier.
__device__ void dime_stage_tile(int64_t t0, int64_t T, int64_t E, int n, int nk,
                                const float* __restrict__ sbe, const float* __restrict__ angle,
                                const int64_t* __restrict__ idx_kj,
                                const float* __restrict__ pref, float* sbL, float* YL,
                                int64_t* kjL) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid < kTile) {
    const int64_t kj = t0 + tid < T ? idx_kj[t0 + tid] : -1;
    kjL[tid] = kj < E ? kj : -1;  // an index outside the edges reads as a zero row
  }
  __syncthreads();
  for (int i = tid; i < kTile * nk; i += nt) {
    const int r = i / nk, c = i - r * nk;
    const int64_t kj = kjL[r];
    sbL[c * kLd + r] = kj >= 0 ? sbe[kj * nk + c] : 0.f;
  }
  if (tid < kTile) {
    if (t0 + tid < T) {
      legendre_m0<false>(n, angle[t0 + tid], pref, YL + tid, kLd);
    } else {
      for (int l = 0; l < n; ++l) YL[l * kLd + tid] = 0.f;
    }
  }
  __syncthreads();
}

// one wave per tile, lane = triplet.  wt (n k, o_ld): feature-major, columns o = layer * b + j,
// the leading dimension padded to a multiple of kOC with zeros.
__global__ __launch_bounds__(kTile) void dime_triplet_proj_fwd(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ sbe,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ wt, int O, int o_ld, int b,
    float* __restrict__ S) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k;
  float* sbL = sm;
  float* YL = sm + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    dime_stage_tile(t0, T, E, n, nk, sbe, angle, idx_kj, pref, sbL, YL, kjL);
    const int64_t t = t0 + lane;
    for (int o0 = 0; o0 < O; o0 += kOC) {
      float acc[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
      for (int l = 0; l < n; ++l) {
        const float y = YL[l * kLd + lane];
        for (int q = 0; q < k; ++q) {
          const int f = l * k + q;
          const float e = sbL[f * kLd + lane] * y;
          const float* w = wt + (int64_t)f * o_ld + o0;
#pragma unroll
          for (int u = 0; u < kOC; ++u) acc[u] = fmaf(w[u], e, acc[u]);
        }
      }
      if (t < T) {
#pragma unroll
        for (int u = 0; u < kOC; ++u) {
          const int o = o0 + u;
          if (o < O) S[((int64_t)(o / b) * T + t) * b + o % b] = acc[u];
        }
      }
    }
  }
}

// the materialising form: sbf (T, n k)
__global__ __launch_bounds__(kTile) void dime_triplet_emb(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ sbe,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, float* __restrict__ sbf) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k;
  float* sbL = sm;
  float* YL = sm + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    dime_stage_tile(t0, T, E, n, nk, sbe, angle, idx_kj, pref, sbL, YL, kjL);
    for (int r = 0; r < kTile && t0 + r < T; ++r)
      for (int f = lane; f < nk; f += kTile)
        sbf[(t0 + r) * nk + f] = sbL[f * kLd + r] * YL[(f / k) * kLd + r];
  }
}

// Weight gradients: block b sums its contiguous range of tiles, thread = feature, blockIdx.y =
// chunk of kOC output columns; triplets are added in index order.  One partial row per block.
__global__ void dime_triplet_proj_wgrad(
    int64_t T, int64_t E, int n, int k, int64_t tiles_per_block, const float* __restrict__ sbe,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ gS, int O, int o_ld, int b,
    float* __restrict__ partials) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  __shared__ float gL[kTile][kOC];
  const int nk = n * k;
  float* sbL = sm;
  float* YL = sm + nk * kLd;
  const int tid = threadIdx.x;
  const int o0 = blockIdx.y * kOC;
  const int f = tid;
  const bool active = f < nk;
  const int yrow = active ? f / k : 0, srow = active ? f : 0;
  float acc[kOC];
#pragma unroll
  for (int u = 0; u < kOC; ++u) acc[u] = 0.f;
  const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_block;
  for (int64_t tile = tile0; tile < tile0 + tiles_per_block; ++tile) {
    const int64_t t0 = tile * kTile;
    if (t0 >= T) break;
    __syncthreads();
    dime_stage_tile(t0, T, E, n, nk, sbe, angle, idx_kj, pref, sbL, YL, kjL);
    for (int i = tid; i < kTile * kOC; i += blockDim.x) {
      const int r = i / kOC, u = i % kOC;
      const int o = o0 + u;
      const int64_t t = t0 + r;
      gL[r][u] = (t < T && o < O) ? gS[((int64_t)(o / b) * T + t) * b + o % b] : 0.f;
    }
    __syncthreads();
    if (active) {
      for (int r = 0; r < kTile; ++r) {
        const float e = sbL[srow * kLd + r] * YL[yrow * kLd + r];
#pragma unroll
        for (int u = 0; u < kOC; ++u) acc[u] = fmaf(gL[r][u], e, acc[u]);
      }
    }
  }
  if (active) {
    float* row = partials + (int64_t)blockIdx.x * nk * o_ld;
#pragma unroll
    for (int u = 0; u < kOC; ++u) row[(int64_t)f * o_ld + o0 + u] = acc[u];
  }
}

// Geometry gradients: lane = triplet; g_sbf[f] = sum_o w[f, o] g[o] is folded at once into
// g_sbe (per-triplet rows, summed per edge by the caller over the CSR of idx_kj) and g_Y, which
// the Legendre derivatives turn into g_angle.
__global__ __launch_bounds__(kTile) void dime_triplet_proj_geom_bwd(
    int64_t T, int64_t E, int n, int k, const float* __restrict__ sbe,
    const float* __restrict__ angle, const int64_t* __restrict__ idx_kj,
    const float* __restrict__ pref, const float* __restrict__ wt, int O, int o_ld, int b,
    const float* __restrict__ gS, float* __restrict__ g_sbe_rows, float* __restrict__ g_angle) {
  extern __shared__ float sm[];
  __shared__ int64_t kjL[kTile];
  const int nk = n * k;
  float* sbL = sm;
  float* YL = sm + nk * kLd;
  float* gsL = YL + n * kLd;
  float* gyL = gsL + nk * kLd;
  const int lane = threadIdx.x;
  for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < T; t0 += (int64_t)gridDim.x * kTile) {
    __syncthreads();
    dime_stage_tile(t0, T, E, n, nk, sbe, angle, idx_kj, pref, sbL, YL, kjL);
    const int64_t t = t0 + lane;
    for (int i = 0; i < nk; ++i) gsL[i * kLd + lane] = 0.f;
    for (int i = 0; i < n; ++i) gyL[i * kLd + lane] = 0.f;
    for (int o0 = 0; o0 < O; o0 += kOC) {
      float g[kOC];
#pragma unroll
      for (int u = 0; u < kOC; ++u) {
        const int o = o0 + u;
        g[u] = (t < T && o < O) ? gS[((int64_t)(o / b) * T + t) * b + o % b] : 0.f;
      }
      for (int l = 0; l < n; ++l) {
        const float y = YL[l * kLd + lane];
        float gy = 0.f;
        for (int q = 0; q < k; ++q) {
          const int f = l * k + q;
          const float* w = wt + (int64_t)f * o_ld + o0;
          float ge = 0.f;
#pragma unroll
          for (int u = 0; u < kOC; ++u) ge = fmaf(w[u], g[u], ge);
          gsL[f * kLd + lane] += ge * y;
          gy = fmaf(ge, sbL[f * kLd + lane], gy);
        }
        gyL[l * kLd + lane] += gy;
      }
    }
    if (t < T) g_angle[t] = legendre_m0<true>(n, angle[t], pref, gyL + lane, kLd);
    __syncthreads();
    for (int r = 0; r < kTile && t0 + r < T; ++r)
      for (int c = lane; c < nk; c += kTile) g_sbe_rows[(t0 + r) * nk + c] = gsL[c * kLd + r];
  }
}

int64_t proj_bwd_blocks(int64_t T) {
  return std::max<int64_t>(1, std::min<int64_t>(ceil_div(T, kTile), kProjBwdBlocks));
}

unsigned tile_grid(int64_t T) {
  return (unsigned)std::min<int64_t>(ceil_div(T, kTile), (int64_t)1 << 20);
}

bool basis_ok(int n, int k) { return n >= 1 && k >= 1 && n <= 16 && k <= 64; }

// ------------------------------------------------------------------------------------- K19d
// lane r's value of v in every lane, as a wave-uniform (scalar) value: r is the same in all
// lanes, so what is indexed by the result is addressed once per wave
__device__ __forceinline__ long long wave_bcast(long long v, int r) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), r);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), r);
  return ((long long)hi << 32) | (long long)lo;
}

// out[s, c] = sum_{p in [rowptr[s], rowptr[s+1])} src[gidx[t], c] (W S_t)[c], t = perm[p] (or p);
// sW[j * I + c] = W[c * b + j]
__global__ __launch_bounds__(kWaves * kWave) void interact1_fwd(
    int64_t n_seg, int64_t n_src, int64_t T, int I, int b, const float* __restrict__ src,
    const float* __restrict__ S, const float* __restrict__ W, const int64_t* __restrict__ gidx,
    const int64_t* __restrict__ perm, const int64_t* __restrict__ rowptr,
    float* __restrict__ out) {
  extern __shared__ float sW[];
  for (int i = threadIdx.x; i < I * b; i += blockDim.x) {
    const int c = i / b, j = i - c * b;
    sW[j * I + c] = W[i];
  }
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  // the wave's index as a scalar: the segment, its range and every triplet index below are then
  // wave-uniform to the compiler (scalar loads and branches)
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t s = (int64_t)blockIdx.x * kWaves + wv;
  if (s >= n_seg) return;
  const int64_t p0 = rowptr[s], p1 = rowptr[s + 1];
  for (int c0 = 0; c0 < I; c0 += kWave) {
    const int c = c0 + lane;
    const bool cok = c < I;
    float acc = 0.f;
    for (int64_t pb = p0; pb < p1; pb += kWave) {
      // the (triplet, source row) pairs of the next kWave entries in two coalesced loads,
      // handed out lane by lane as wave-uniform values; -1 = contributes nothing
      long long tl = -1, gl = -1;
      if (pb + lane < p1) {
        const int64_t t = perm ? perm[pb + lane] : pb + lane;
        if (t >= 0 && t < T) {
          const int64_t g = gidx[t];
          if (g >= 0 && g < n_src) tl = t, gl = g;
        }
      }
      const int cnt = (int)std::min<int64_t>(kWave, p1 - pb);
      for (int r = 0; r < cnt; ++r) {
        const int64_t t = wave_bcast(tl, r);
        if (t < 0) continue;
        const int64_t g = wave_bcast(gl, r);
        float a = 0.f;
        for (int j = 0; j < b; ++j) a = fmaf(cok ? sW[j * I + c] : 0.f, S[t * b + j], a);
        acc = fmaf(cok ? src[g * I + c] : 0.f, a, acc);
      }
    }
    if (cok) out[s * I + c] = acc;
  }
}

// v[j], j < kB, per lane -> the sum over the 64 lanes of v[j], returned in every lane of the
// group of 64 / kB lanes whose upper lane bits spell j (bit 5 the highest bit of j): each of the
// log2(kB) exchange steps halves the values a lane carries, then the remaining lane bits are
// summed by a plain butterfly.  kB - 1 + log2(64 / kB) shuffles instead of 6 kB.
template <int kB>
__device__ __forceinline__ float transpose_sum(float (&v)[kB], int lane) {
  int off = kWave / 2;
#pragma unroll
  for (int half = kB / 2; half >= 1; half /= 2, off /= 2) {
    const bool upper = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = upper ? v[i] : v[i + half];
      const float keep = upper ? v[i + half] : v[i];
      v[i] = keep + __shfl_xor(send, off, kWave);
    }
  }
  float r = v[0];
  for (; off >= 1; off /= 2) r += __shfl_xor(r, off, kWave);
  return r;
}

// Wave w of the grid owns edges [w * epw, (w + 1) * epw); lane = channel of the 64-channel chunk
// c0.  Per triplet u[c] = grad_m[e, c] xd[idx_kj[t], c]; grad_w[c, j] += u[c] S_t[j] stays in kB
// registers per lane, grad_S[t, j] = sum_c W[c, j] u[c] by transpose_sum.  Chunks past the first
// (I > 64) walk the wave's triplets again and add their part of grad_S to what the wave itself
// wrote before (same lane, same address: ordered).  One partial row (I, b) per wave.
template <int kB>
__global__ __launch_bounds__(kWaves * kWave) void interact1_bwd(
    int64_t E, int64_t T, int64_t epw, int I, int b, const float* __restrict__ gm,
    const float* __restrict__ xd, const float* __restrict__ S, const float* __restrict__ W,
    const int64_t* __restrict__ idx_kj, const int64_t* __restrict__ offs, float* gS,
    float* __restrict__ partials) {
  constexpr int kGroup = kWave / kB;  // lanes that end up with the same column of grad_S
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);  // scalar, as in the forward
  const int lane = threadIdx.x % kWave;
  const int64_t gw = (int64_t)blockIdx.x * kWaves + wv;
  const int64_t e0 = std::min<int64_t>(gw * epw, E), e1 = std::min<int64_t>(e0 + epw, E);
  const int jcol = lane / kGroup;
  const bool writer = lane % kGroup == 0 && jcol < b;
  float* row = partials + gw * (int64_t)I * b;
  for (int c0 = 0; c0 < I; c0 += kWave) {
    const int c = c0 + lane;
    const bool cok = c < I;
    float w[kB], acc[kB];
#pragma unroll
    for (int j = 0; j < kB; ++j) {
      w[j] = (cok && j < b) ? W[(int64_t)c * b + j] : 0.f;
      acc[j] = 0.f;
    }
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t t0 = std::max<int64_t>(offs[e], 0), t1 = std::min<int64_t>(offs[e + 1], T);
      if (t0 >= t1) continue;
      const float g = cok ? gm[e * I + c] : 0.f;  // the same for every triplet of the edge
      for (int64_t tb = t0; tb < t1; tb += kWave) {
        // idx_kj of the next kWave triplets in one coalesced load, handed out lane by lane; the
        // xd row of triplet r + 1 is requested before triplet r is worked on
        const long long kjv = tb + lane < t1 ? (long long)idx_kj[tb + lane] : -1;
        const int cnt = (int)std::min<int64_t>(kWave, t1 - tb);
        auto xd_of = [&](int r) {
          const int64_t kj = wave_bcast(kjv, r);
          return (kj >= 0 && kj < E && cok) ? xd[kj * I + c] : 0.f;
        };
        float x_next = xd_of(0);
        for (int r = 0; r < cnt; ++r) {
          const int64_t t = tb + r;
          const float u = g * x_next;
          if (r + 1 < cnt) x_next = xd_of(r + 1);
          float gs[kB];
#pragma unroll
          for (int j = 0; j < kB; ++j) {
            const float s = j < b ? S[t * b + j] : 0.f;
            acc[j] = fmaf(u, s, acc[j]);
            gs[j] = w[j] * u;
          }
          const float v = transpose_sum<kB>(gs, lane);
          if (writer) {
            float* dst = gS + t * b + jcol;
            *dst = c0 == 0 ? v : *dst + v;
          }
        }
      }
    }
    if (cok) {
#pragma unroll
      for (int j = 0; j < kB; ++j)
        if (j < b) row[(int64_t)c * b + j] = acc[j];
    }
  }
}

int64_t bwd_blocks(int64_t E) {
  return std::max<int64_t>(1, std::min<int64_t>(ceil_div(E, kWaves), kBwdBlocks));
}

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int64_t gmp_dime_edge_basis_bwd_partial_rows(int64_t n_edges) {
  return n_edges > 0 ? ceil_div(n_edges, kEdgeT) : 0;
}

int gmp_dime_edge_basis_fwd_f32(const float* dist, int64_t n_edges, float cutoff,
                                int envelope_exponent, const float* freq, int num_radial,
                                const float* zeros, const float* norm, int num_spherical,
                                float* rbf, float* sbe, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0);
  if (n_edges == 0) return GMP_OK;
  GMP_CHECK_ARG(dist && freq && zeros && norm && rbf && sbe);
  const int nk = num_spherical * num_radial;
  const int64_t total = n_edges * (num_radial + nk);
  GMP_CHECK_ARG(ceil_div(total, kEdgeT) <= INT32_MAX);
  dime_edge_basis_fwd<<<(unsigned)ceil_div(total, kEdgeT), kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm, nk, rbf, sbe);
  return launch_status();
}

int gmp_dime_edge_basis_bwd_f32(const float* dist, int64_t n_edges, float cutoff,
                                int envelope_exponent, const float* freq, int num_radial,
                                const float* zeros, const float* norm, int num_spherical,
                                const float* grad_rbf, const float* grad_sbe, float* grad_dist,
                                float* grad_freq, float* freq_partials, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && basis_ok(num_spherical, num_radial) && cutoff > 0.f &&
                envelope_exponent >= 0 && grad_freq);
  if (n_edges == 0)
    return hip_check(hipMemsetAsync(grad_freq, 0, num_radial * sizeof(float), as_stream(stream)));
  GMP_CHECK_ARG(dist && freq && zeros && norm && grad_dist && freq_partials);
  const int64_t nb = ceil_div(n_edges, kEdgeT);
  GMP_CHECK_ARG(nb <= INT32_MAX);
  dime_edge_basis_bwd<<<(unsigned)nb, kEdgeT, 0, as_stream(stream)>>>(
      dist, n_edges, cutoff, envelope_exponent, freq, num_radial, zeros, norm,
      num_spherical * num_radial, grad_rbf, grad_sbe, grad_dist, freq_partials);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  return gmp_sum_rows_f32(freq_partials, nb, num_radial, grad_freq, stream);
}

int gmp_dime_triplet_proj_fwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                  int num_radial, const float* sbe, const float* angle,
                                  const int64_t* idx_kj, const float* pref, const float* w_sbf1_t,
                                  int n_layers, int b, float* S, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(num_spherical, num_radial) &&
                n_layers >= 1 && b >= 1);
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(sbe && angle && idx_kj && pref && w_sbf1_t && S && n_edges > 0);
  const int O = n_layers * b, o_ld = (int)ceil_div(O, kOC) * kOC;
  const size_t lds = (size_t)(num_spherical * num_radial + num_spherical) * kLd * sizeof(float);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  dime_triplet_proj_fwd<<<tile_grid(n_triplets), kTile, lds, as_stream(stream)>>>(
      n_triplets, n_edges, num_spherical, num_radial, sbe, angle, idx_kj, pref, w_sbf1_t, O, o_ld,
      b, S);
  return launch_status();
}

int gmp_dime_triplet_emb_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                             int num_radial, const float* sbe, const float* angle,
                             const int64_t* idx_kj, const float* pref, float* sbf, void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(num_spherical, num_radial));
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(sbe && angle && idx_kj && pref && sbf && n_edges > 0);
  const size_t lds = (size_t)(num_spherical * num_radial + num_spherical) * kLd * sizeof(float);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  dime_triplet_emb<<<tile_grid(n_triplets), kTile, lds, as_stream(stream)>>>(
      n_triplets, n_edges, num_spherical, num_radial, sbe, angle, idx_kj, pref, sbf);
  return launch_status();
}

int64_t gmp_dime_triplet_proj_bwd_partial_rows(int64_t n_triplets) {
  return proj_bwd_blocks(n_triplets);
}

int gmp_dime_triplet_proj_bwd_f32(int64_t n_triplets, int64_t n_edges, int num_spherical,
                                  int num_radial, const float* sbe, const float* angle,
                                  const int64_t* idx_kj, const float* pref, const float* w_sbf1_t,
                                  int n_layers, int b, const float* grad_S, float* grad_w,
                                  float* partials, float* grad_sbe_rows, float* grad_angle,
                                  void* stream) {
  GMP_CHECK_ARG(n_triplets >= 0 && n_edges >= 0 && basis_ok(num_spherical, num_radial) &&
                n_layers >= 1 && b >= 1 && grad_w);
  const int n = num_spherical, k = num_radial, nk = n * k;
  const int O = n_layers * b, o_ld = (int)ceil_div(O, kOC) * kOC;
  const int64_t width = (int64_t)nk * o_ld;
  hipStream_t s = as_stream(stream);
  if (n_triplets == 0) return hip_check(hipMemsetAsync(grad_w, 0, width * sizeof(float), s));
  GMP_CHECK_ARG(sbe && angle && idx_kj && pref && w_sbf1_t && grad_S && partials && n_edges > 0);
  const int threads = (int)ceil_div(nk, kWave) * kWave;
  const size_t lds = (size_t)(nk + n) * kLd * sizeof(float);
  if (threads > 1024 || lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = proj_bwd_blocks(n_triplets);
  const int64_t tpb = ceil_div(ceil_div(n_triplets, kTile), nb);
  dime_triplet_proj_wgrad<<<dim3((unsigned)nb, (unsigned)(o_ld / kOC)), threads, lds, s>>>(
      n_triplets, n_edges, n, k, tpb, sbe, angle, idx_kj, pref, grad_S, O, o_ld, b, partials);
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  rc = gmp_sum_rows_f32(partials, nb, width, grad_w, stream);
  if (rc != GMP_OK) return rc;
  if (grad_sbe_rows || grad_angle) {
    GMP_CHECK_ARG(grad_sbe_rows && grad_angle);
    if (2 * lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
    dime_triplet_proj_geom_bwd<<<tile_grid(n_triplets), kTile, 2 * lds, s>>>(
        n_triplets, n_edges, n, k, sbe, angle, idx_kj, pref, w_sbf1_t, O, o_ld, b, grad_S,
        grad_sbe_rows, grad_angle);
    rc = launch_status();
  }
  return rc;
}

int gmp_triplet_interact1_fwd_f32(int64_t n_seg, int64_t n_src, int64_t n_triplets, int64_t I,
                                  int b, const float* src, const float* S, const float* w_sbf2,
                                  const int64_t* gather_idx, const int64_t* perm,
                                  const int64_t* rowptr, float* out, void* stream) {
  GMP_CHECK_ARG(n_seg >= 0 && n_src >= 0 && n_triplets >= 0 && I >= 1 && I <= INT32_MAX &&
                b >= 1);
  if (n_seg == 0) return GMP_OK;
  GMP_CHECK_ARG(w_sbf2 && rowptr && out);
  GMP_CHECK_ARG(n_triplets == 0 || (src && S && gather_idx));
  const size_t lds = (size_t)I * b * sizeof(float);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = ceil_div(n_seg, kWaves);
  GMP_CHECK_ARG(nb <= INT32_MAX);
  interact1_fwd<<<(unsigned)nb, kWaves * kWave, lds, as_stream(stream)>>>(
      n_seg, n_src, n_triplets, (int)I, b, src, S, w_sbf2, gather_idx, perm, rowptr, out);
  return launch_status();
}

int64_t gmp_triplet_interact1_bwd_partial_rows(int64_t n_edges) {
  return bwd_blocks(n_edges) * kWaves;
}

int gmp_triplet_interact1_bwd_f32(int64_t n_edges, int64_t n_triplets, int64_t I, int b,
                                  const float* grad_m, const float* xd, const float* S,
                                  const float* w_sbf2, const int64_t* idx_kj,
                                  const int64_t* offsets, float* grad_S, float* grad_w,
                                  float* partials, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0 && I >= 1 && I <= INT32_MAX && b >= 1 &&
                b <= kMaxB && grad_w);
  hipStream_t s = as_stream(stream);
  const int64_t nw = I * b;
  if (n_edges == 0 || n_triplets == 0)
    return hip_check(hipMemsetAsync(grad_w, 0, nw * sizeof(float), s));
  GMP_CHECK_ARG(grad_m && xd && S && w_sbf2 && idx_kj && offsets && grad_S && partials);
  // the forward's cap (its weights live in LDS), so that both directions accept the same sizes
  if ((size_t)nw * sizeof(float) > kLdsCap) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = bwd_blocks(n_edges);
  const int64_t epw = ceil_div(n_edges, nb * kWaves);
  if (b <= 8) {
    interact1_bwd<8><<<(unsigned)nb, kWaves * kWave, 0, s>>>(
        n_edges, n_triplets, epw, (int)I, b, grad_m, xd, S, w_sbf2, idx_kj, offsets, grad_S,
        partials);
  } else {
    interact1_bwd<kMaxB><<<(unsigned)nb, kWaves * kWave, 0, s>>>(
        n_edges, n_triplets, epw, (int)I, b, grad_m, xd, S, w_sbf2, idx_kj, offsets, grad_S,
        partials);
  }
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  return gmp_sum_rows_f32(partials, nb * kWaves, nw, grad_w, stream);
}

}  // extern "C"
