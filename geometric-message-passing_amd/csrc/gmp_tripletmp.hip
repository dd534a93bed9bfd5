// K19: SphereNet's triplet interaction (spherenet_layer.py update_e.forward: x_kj[idx_kj] * sbf
// * t, then scatter over idx_ji) for one layer, without the (T, I) messages in HBM:
//
//   m[e, c] = sum_{t in [offs[e], offs[e+1])} xd[idx_kj[t], c] (W_sbf2 S_t)[c] (W_t2 P_t)[c]
//
// K11 emits the triplets of one edge j -> i contiguously, so `offs` is a row pointer and one
// wave walks one edge's triplets in index order with lane = channel: no atomics, and the sum
// order is fixed, so two runs agree bit for bit.  The same kernel run over the CSR of idx_kj
// (rows through `perm`, gathering grad_m by idx_ji) is the gradient of xd.
// The backward walks contiguous edge ranges per wave: g_S / g_P by a butterfly over the
// channels, the second projections' weight gradients as one partial row per wave, summed in
// wave order afterwards.
//
// K19d: DimeNet++'s form of the same (PyG 2.3.1 InteractionPPBlock), without the torsion factor:
//
//   m[e, c] = sum_{t in [offs[e], offs[e+1])} xd[idx_kj[t], c] (W_sbf2 S_t)[c]
//
// The walk, the constants and the launch shapes are K19's.  Its gradient kernel is a different
// algorithm: the weight-gradient accumulators stay in registers (lane = channel) and the b
// per-triplet sums of grad_S are reduced by one transposing butterfly.
#include <algorithm>

#include "gmp_common.h"

namespace gmp {
namespace {

constexpr int kWaves = 4;            // waves per block
constexpr int kMaxB = 16;            // every basis_emb_size <= kMaxB in the backward kernels
// The backward's grid is capped here (kWaves partial rows each): enough workgroups that the
// dependent index -> row loads of one wave hide behind the other waves of its CU.
constexpr int kBwdBlocks = 2048;
constexpr size_t kLdsCap = 60 * 1024;

// sW[j * I + c] = W[c * b + j]
__device__ void load_wt(const float* __restrict__ W, int I, int b, float* sW) {
  for (int i = threadIdx.x; i < I * b; i += blockDim.x) {
    const int c = i / b, j = i - c * b;
    sW[j * I + c] = W[i];
  }
}

// out[s, c] = sum_{p in [rowptr[s], rowptr[s+1])} src[gidx[t], c] a_t[c] b_t[c], t = perm[p] (or p)
__global__ __launch_bounds__(kWaves * kWave) void interact_fwd(
    int64_t n_seg, int64_t n_src, int64_t T, int I, int ba, int bt, const float* __restrict__ src,
    const float* __restrict__ S, const float* __restrict__ P, const float* __restrict__ Wa,
    const float* __restrict__ Wt, const int64_t* __restrict__ gidx,
    const int64_t* __restrict__ perm, const int64_t* __restrict__ rowptr,
    float* __restrict__ out) {
  extern __shared__ float sm[];
  float* sWa = sm;
  float* sWt = sm + I * ba;
  load_wt(Wa, I, ba, sWa);
  load_wt(Wt, I, bt, sWt);
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  const int64_t s = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
  if (s >= n_seg) return;
  const int64_t p0 = rowptr[s], p1 = rowptr[s + 1];
  for (int c = lane; c < I; c += kWave) {
    float acc = 0.f;
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t t = perm ? perm[p] : p;
      if (t < 0 || t >= T) continue;
      const int64_t g = gidx[t];
      if (g < 0 || g >= n_src) continue;
      float a = 0.f, b = 0.f;
      for (int j = 0; j < ba; ++j) a = fmaf(sWa[j * I + c], S[t * ba + j], a);
      for (int j = 0; j < bt; ++j) b = fmaf(sWt[j * I + c], P[t * bt + j], b);
      acc = fmaf(src[g * I + c], a * b, acc);
    }
    out[s * I + c] = acc;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// wave w of the grid owns edges [w * epw, (w + 1) * epw); kB >= max(ba, bt) sizes the unrolled
// per-triplet registers (kB = 8: half the registers, twice the waves in flight)
template <int kB>
__global__ __launch_bounds__(kWaves * kWave) void interact_bwd(
    int64_t E, int64_t T, int64_t epw, int I, int ba, int bt, const float* __restrict__ gm,
    const float* __restrict__ xd, const float* __restrict__ S, const float* __restrict__ P,
    const float* __restrict__ Wa, const float* __restrict__ Wt,
    const int64_t* __restrict__ idx_kj, const int64_t* __restrict__ offs,
    float* __restrict__ gS, float* __restrict__ gP, float* __restrict__ partials) {
  extern __shared__ float sm[];
  const int nw = I * (ba + bt);
  float* sWa = sm;
  float* sWt = sm + I * ba;
  const int wv = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float* accA = sm + nw + wv * nw;  // [j * I + c], this wave's
  float* accT = accA + I * ba;
  load_wt(Wa, I, ba, sWa);
  load_wt(Wt, I, bt, sWt);
  for (int i = lane; i < nw; i += kWave) accA[i] = 0.f;
  __syncthreads();
  const int64_t gw = (int64_t)blockIdx.x * kWaves + wv;
  const int64_t e0 = std::min<int64_t>(gw * epw, E), e1 = std::min<int64_t>(e0 + epw, E);
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t t0 = std::max<int64_t>(offs[e], 0), t1 = std::min<int64_t>(offs[e + 1], T);
    long long kjv = -1;
    const float gm0 = (t0 < t1 && lane < I) ? gm[e * I + lane] : 0.f;  // the same for every t
    for (int64_t t = t0; t < t1; ++t) {
      // idx_kj of the next kWave triplets in one coalesced load, handed out lane by lane
      const int r = (int)((t - t0) % kWave);
      if (r == 0) kjv = t + lane < t1 ? (long long)idx_kj[t + lane] : -1;
      const int64_t kj = __shfl(kjv, r, kWave);
      const bool ok = kj >= 0 && kj < E;
      float s[kB], q[kB], gs[kB], gq[kB];
#pragma unroll
      for (int j = 0; j < kB; ++j) {
        s[j] = j < ba ? S[t * ba + j] : 0.f;
        q[j] = j < bt ? P[t * bt + j] : 0.f;
        gs[j] = 0.f, gq[j] = 0.f;
      }
      for (int c = lane; c < I; c += kWave) {
        const float u = ok ? (c == lane ? gm0 : gm[e * I + c]) * xd[kj * I + c] : 0.f;
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int j = 0; j < kB; ++j) {
          if (j < ba) a = fmaf(sWa[j * I + c], s[j], a);
          if (j < bt) b = fmaf(sWt[j * I + c], q[j], b);
        }
        const float ga = u * b, gb = u * a;
#pragma unroll
        for (int j = 0; j < kB; ++j) {
          if (j < ba) {
            accA[j * I + c] = fmaf(ga, s[j], accA[j * I + c]);
            gs[j] = fmaf(sWa[j * I + c], ga, gs[j]);
          }
          if (j < bt) {
            accT[j * I + c] = fmaf(gb, q[j], accT[j * I + c]);
            gq[j] = fmaf(sWt[j * I + c], gb, gq[j]);
          }
        }
      }
      float outs = 0.f, outq = 0.f;
#pragma unroll
      for (int j = 0; j < kB; ++j) {
        if (j < ba) {
          const float v = wave_sum(gs[j]);
          if (lane == j) outs = v;
        }
        if (j < bt) {
          const float v = wave_sum(gq[j]);
          if (lane == j) outq = v;
        }
      }
      if (lane < ba) gS[t * ba + lane] = outs;
      if (lane < bt) gP[t * bt + lane] = outq;
    }
  }
  // partial row of this wave: [g_Wa (I, ba) | g_Wt (I, bt)]
  __syncthreads();
  float* row = partials + gw * nw;
  for (int i = lane; i < I * ba; i += kWave) row[i] = accA[(i % ba) * I + i / ba];
  for (int i = lane; i < I * bt; i += kWave) row[I * ba + i] = accT[(i % bt) * I + i / bt];
}

// ------------------------------------------------------------------------------------- K19d
// lane r's value of v in every lane, as a wave-uniform (scalar) value: r is the same in all
// lanes, so what is indexed by the result is addressed once per wave
__device__ __forceinline__ long long wave_bcast(long long v, int r) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(v & 0xffffffffll), r);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), r);
  return ((long long)hi << 32) | (long long)lo;
}

// out[s, c] = sum_{p in [rowptr[s], rowptr[s+1])} src[gidx[t], c] (W S_t)[c], t = perm[p] (or p)
__global__ __launch_bounds__(kWaves * kWave) void interact1_fwd(
    int64_t n_seg, int64_t n_src, int64_t T, int I, int b, const float* __restrict__ src,
    const float* __restrict__ S, const float* __restrict__ W, const int64_t* __restrict__ gidx,
    const int64_t* __restrict__ perm, const int64_t* __restrict__ rowptr,
    float* __restrict__ out) {
  extern __shared__ float sW[];
  load_wt(W, I, b, sW);
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

int gmp_triplet_interact_fwd_f32(int64_t n_seg, int64_t n_src, int64_t n_triplets, int64_t I,
                                 int ba, int bt, const float* src, const float* S, const float* P,
                                 const float* w_sbf2, const float* w_t2, const int64_t* gather_idx,
                                 const int64_t* perm, const int64_t* rowptr, float* out,
                                 void* stream) {
  GMP_CHECK_ARG(n_seg >= 0 && n_src >= 0 && n_triplets >= 0 && I >= 1 && I <= INT32_MAX &&
                ba >= 1 && bt >= 1);
  if (n_seg == 0) return GMP_OK;
  GMP_CHECK_ARG(w_sbf2 && w_t2 && rowptr && out);
  GMP_CHECK_ARG(n_triplets == 0 || (src && S && P && gather_idx));
  const size_t lds = (size_t)I * (ba + bt) * sizeof(float);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = ceil_div(n_seg, kWaves);
  GMP_CHECK_ARG(nb <= INT32_MAX);
  interact_fwd<<<(unsigned)nb, kWaves * kWave, lds, as_stream(stream)>>>(
      n_seg, n_src, n_triplets, (int)I, ba, bt, src, S, P, w_sbf2, w_t2, gather_idx, perm, rowptr,
      out);
  return launch_status();
}

int64_t gmp_triplet_interact_bwd_partial_rows(int64_t n_edges) {
  return bwd_blocks(n_edges) * kWaves;
}

int gmp_triplet_interact_bwd_f32(int64_t n_edges, int64_t n_triplets, int64_t I, int ba, int bt,
                                 const float* grad_m, const float* xd, const float* S,
                                 const float* P, const float* w_sbf2, const float* w_t2,
                                 const int64_t* idx_kj, const int64_t* offsets, float* grad_S,
                                 float* grad_P, float* grad_w, float* partials, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0 && I >= 1 && I <= INT32_MAX && ba >= 1 &&
                bt >= 1 && ba <= kMaxB && bt <= kMaxB && grad_w);
  hipStream_t s = as_stream(stream);
  const int64_t nw = I * (ba + bt);
  if (n_edges == 0 || n_triplets == 0)
    return hip_check(hipMemsetAsync(grad_w, 0, nw * sizeof(float), s));
  GMP_CHECK_ARG(grad_m && xd && S && P && w_sbf2 && w_t2 && idx_kj && offsets && grad_S &&
                grad_P && partials);
  const size_t lds = (size_t)nw * (1 + kWaves) * sizeof(float);
  if (lds > kLdsCap) return GMP_ERR_UNSUPPORTED;
  const int64_t nb = bwd_blocks(n_edges);
  const int64_t epw = ceil_div(n_edges, nb * kWaves);
  if (ba <= 8 && bt <= 8) {
    interact_bwd<8><<<(unsigned)nb, kWaves * kWave, lds, s>>>(
        n_edges, n_triplets, epw, (int)I, ba, bt, grad_m, xd, S, P, w_sbf2, w_t2, idx_kj, offsets,
        grad_S, grad_P, partials);
  } else {
    interact_bwd<kMaxB><<<(unsigned)nb, kWaves * kWave, lds, s>>>(
        n_edges, n_triplets, epw, (int)I, ba, bt, grad_m, xd, S, P, w_sbf2, w_t2, idx_kj, offsets,
        grad_S, grad_P, partials);
  }
  int rc = launch_status();
  if (rc != GMP_OK) return rc;
  return gmp_sum_rows_f32(partials, nb * kWaves, nw, grad_w, stream);
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
