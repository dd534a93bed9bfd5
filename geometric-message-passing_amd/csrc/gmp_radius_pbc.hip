// K9p: radius graph under periodic boundary conditions.  The contract (which (j -> i, S) are
// edges, the fp32 formula that decides it, the output order) is stated once, in include/gmp.h;
// this file is the cells -> count -> cumsum -> fill shape of K9 (gmp_radius.hip) over bins in
// fractional coordinates.
//
// Binning.  Per graph the host plans, in fp64, nb_k bins along lattice axis k and a reach m_k
// with (h_k / nb_k) * m_k >= r (1 + eps), h_k the perpendicular height of the cell along k.  A
// node's fractional coordinate is f_k = ((p0 inv[0][k] + p1 inv[1][k]) + p2 inv[2][k]) in fp32.
// On a periodic axis w_k = floor(f_k) is the node's wrap and its bin floor((f_k - w_k) nb_k),
// clamped to nb_k - 1; the node then counts as lying in the unwrapped bin W_k = w_k nb_k + bin.
// On a non-periodic axis w_k = 0 and the bin is floor((f_k - org_k) scale_k) clamped to
// [0, nb_k), org / scale spanning the graph's fractional bounding box.
//
// Margin.  Two positions closer than r differ along axis k by less than r nb_k / h_k <=
// m_k / (1 + eps) bin widths.  The fp32 bin coordinate of a node is off its exact value by at
// most delta_k = 12 u A_k scale_k bin widths (u = 2^-24; A_k = max(1, sum_d max|p_d|
// |inv[d][k]|) bounds every partial sum of f_k; the 12 counts the rounding of inv to fp32, of the
// three products and two sums, of f - w and of the scaling, with room to spare).  So the
// computed coordinates differ by less than m_k / (1 + eps) + 2 delta_k, which stays below m_k
// while 2 delta_k <= eps / (1 + eps): with eps = 1e-3 that is A_k scale_k <= 698, i.e. |frac|
// up to ~700 / nb_k for a well-conditioned cell.  The host refuses inputs beyond that bound.
// Numbers closer than m differ in their floors by at most m (clamping only shrinks the
// difference), so every pair within r has |W_i - (W_j + S nb)| <= m for its S and is scanned.
//
// Scan.  One wave per target i.  For delta in [-m, m]^3 (clipped, unwrapped, on non-periodic
// axes) the bin c = bin_i + delta has image q = floor(c / nb) and wrapped bin c - q nb; a node j
// found there is the candidate (j, S = q - w_j + w_i), met exactly once over all delta.  Along
// the fastest axis the bins of one image are consecutive in the bin table, so the wave takes
// them as one range, lanes striding over the nodes.  Each candidate is accepted or rejected by
// the contract's formula on the unwrapped pos, never on wrapped coordinates.
//
// Ordering.  Accepted (j, S) pack into one key j << 24 | (S0 + 128) << 16 | (S1 + 128) << 8 |
// (S2 + 128), whose integer order is the (j, S0, S1, S2) order, and keys are unique.  The wave
// appends its target's keys to LDS (ballot compaction) and sorts them there with a bitonic
// network; a target with more than kCap keys writes them to its range of src_out instead and
// one block sorts that range in place in global memory (gmp_radius_pbc_sort).  Both use the
// all-ascending form of the network (first step of each merge mirrored), where a comparator
// whose upper index is past the end is a no-op, so no padding is stored.
#include "gmp_common.h"

// The contract's arithmetic: every operation rounded to nearest, nothing fused.  HIP's
// __fmul_rn / __fadd_rn are plain operators that the compiler's default contraction may still
// fuse, so contraction is switched off for this file and the formulas use these helpers.
#pragma clang fp contract(off)

namespace gmp {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int kPT = 256;          // threads per block: 4 waves, one target each
constexpr int kCap = 1024;        // keys per wave sorted in LDS (4 * 8 KiB per block)
constexpr int kGI = 8, kGF = 24;  // ints / floats per graph in graph_i / graph_f

// graph_i[b]: nb[3], m[3], periodic mask, 0.   graph_f[b]: inv[9] (f_k = sum_d p_d inv[3 d + k]),
// org[3], scale[3], cell[9] (row-major, rows = lattice vectors)
struct GraphPlan {
  int nb[3], m[3], pmask;
  int64_t base;
};

__device__ __forceinline__ GraphPlan load_plan(const int* __restrict__ gi,
                                               const int64_t* __restrict__ gbase, int64_t b) {
  GraphPlan P;
  const int* g = gi + kGI * b;
  for (int k = 0; k < 3; ++k) {
    P.nb[k] = g[k];
    P.m[k] = g[3 + k];
  }
  P.pmask = g[6];
  P.base = gbase[b];
  return P;
}

__device__ __forceinline__ int pack_wrap(int w0, int w1, int w2) {
  return (w0 + 128) | ((w1 + 128) << 8) | ((w2 + 128) << 16);
}

__global__ void pbc_bin_kernel(const float* __restrict__ pos, const int64_t* __restrict__ batch,
                               int64_t N, int64_t B, const int* __restrict__ gi,
                               const float* __restrict__ gf, const int64_t* __restrict__ gbase,
                               int64_t* __restrict__ bin_out, int* __restrict__ wrap_out,
                               int* __restrict__ err) {
  for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < N;
       a += (int64_t)gridDim.x * blockDim.x) {
    int64_t b = batch ? batch[a] : 0;
    if (b < 0 || b >= B) {  // bad batch entry: park the node in graph 0 and report
      *err = 1;
      b = 0;
    }
    const GraphPlan P = load_plan(gi, gbase, b);
    const float* F = gf + kGF * b;
    const float p0 = pos[3 * a], p1 = pos[3 * a + 1], p2 = pos[3 * a + 2];
    int c[3], w[3];
    for (int k = 0; k < 3; ++k) {
      const float f = add_rn(add_rn(mul_rn(p0, F[k]), mul_rn(p1, F[3 + k])), mul_rn(p2, F[6 + k]));
      float u;
      if ((P.pmask >> k) & 1) {
        const float fl = floorf(f);
        if (!(fabsf(fl) <= 127.f)) *err = 1;  // also NaN
        w[k] = fabsf(fl) <= 127.f ? (int)fl : 0;
        u = mul_rn(sub_rn(f, fl), F[12 + k]);
      } else {
        w[k] = 0;
        u = mul_rn(sub_rn(f, F[9 + k]), F[12 + k]);
      }
      int ci = u >= 0.f ? (int)fminf(floorf(u), 2147483000.f) : 0;
      c[k] = ci >= P.nb[k] ? P.nb[k] - 1 : ci;
    }
    bin_out[a] = P.base + ((int64_t)c[2] * P.nb[1] + c[1]) * P.nb[0] + c[0];
    wrap_out[a] = pack_wrap(w[0], w[1], w[2]);
  }
}

__device__ __forceinline__ int floor_div(int a, int n) {
  const int q = a / n;
  return (a % n != 0 && a < 0) ? q - 1 : q;
}

// the contract's test for the edge (j -> i, S) with cell rows c (9 floats)
__device__ __forceinline__ bool within(const float* pi, const float* __restrict__ pos, int64_t j,
                                       const float* c, int s0, int s1, int s2, float r2) {
  const float f0 = (float)s0, f1 = (float)s1, f2 = (float)s2;
  float d[3];
  for (int k = 0; k < 3; ++k) {
    const float t = add_rn(add_rn(mul_rn(f0, c[k]), mul_rn(f1, c[3 + k])), mul_rn(f2, c[6 + k]));
    d[k] = sub_rn(sub_rn(pi[k], pos[3 * j + k]), t);
  }
  return add_rn(add_rn(mul_rn(d[0], d[0]), mul_rn(d[1], d[1])), mul_rn(d[2], d[2])) < r2;
}

__device__ __forceinline__ void fence_wave() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Comparator `t` of step (k, j) of the all-ascending bitonic network on n keys: j == k / 2 is
// the mirrored first step of the merge of blocks of k, smaller j the half-cleaners.
__device__ __forceinline__ void bitonic_cmp(int64_t* a, int n, int k, int j, int t) {
  int lo, hi;
  if (j == (k >> 1)) {
    const int blk = t / j, off = t - blk * j;
    lo = blk * k + off;
    hi = blk * k + k - 1 - off;
  } else {
    lo = 2 * j * (t / j) + (t % j);
    hi = lo + j;
  }
  if (hi < n) {
    const int64_t x = a[lo], y = a[hi];
    if (x > y) {
      a[lo] = y;
      a[hi] = x;
    }
  }
}

__device__ __forceinline__ void emit_edge(int64_t key, int64_t slot, int64_t* __restrict__ src,
                                          int* __restrict__ sidx) {
  src[slot] = key >> 24;
  sidx[3 * slot] = (int)((key >> 16) & 255) - 128;
  sidx[3 * slot + 1] = (int)((key >> 8) & 255) - 128;
  sidx[3 * slot + 2] = (int)(key & 255) - 128;
}

// MODE 0: counts[i] = number of edges into i.  MODE 1: the edges of target i, sorted, at
// offs[i] (more than kCap of them: packed keys, unsorted, left in src for the sort kernel).
template <int MODE>
__global__ __launch_bounds__(kPT) void pbc_scan_kernel(
    const float* __restrict__ pos, const int64_t* __restrict__ batch, int64_t N, int64_t B,
    float r2, const int* __restrict__ gi, const float* __restrict__ gf,
    const int64_t* __restrict__ gbase, const int64_t* __restrict__ bin,
    const int* __restrict__ wrap, const int64_t* __restrict__ crow,
    const int64_t* __restrict__ cperm, int64_t* __restrict__ counts,
    const int64_t* __restrict__ offs, int64_t* __restrict__ src, int* __restrict__ sidx,
    int* __restrict__ err) {
  __shared__ int64_t s_keys[MODE ? (kPT / 64) * kCap : 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; i < N; i += n_waves) {
    int64_t b = batch ? batch[i] : 0;
    if (b < 0 || b >= B) b = 0;
    const GraphPlan P = load_plan(gi, gbase, b);
    float cell[9];
    for (int k = 0; k < 9; ++k) cell[k] = gf[kGF * b + 15 + k];
    const float pi[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    const int64_t lb = bin[i] - P.base;
    const int bi[3] = {(int)(lb % P.nb[0]), (int)((lb / P.nb[0]) % P.nb[1]),
                       (int)(lb / ((int64_t)P.nb[0] * P.nb[1]))};
    const int wi = wrap[i];
    const int wi0 = (wi & 255) - 128, wi1 = ((wi >> 8) & 255) - 128, wi2 = ((wi >> 16) & 255) - 128;
    const bool per0 = P.pmask & 1, per1 = P.pmask & 2, per2 = P.pmask & 4;
    const int64_t base = MODE ? offs[i] : 0;
    const int64_t deg = MODE ? offs[i + 1] - base : 0;
    const bool in_lds = deg <= kCap;
    int64_t* keys = MODE ? (in_lds ? s_keys + wv * kCap : src + base) : nullptr;
    int64_t filled = 0;  // wave-uniform
    for (int z = bi[2] - P.m[2]; z <= bi[2] + P.m[2]; ++z) {
      if (!per2 && (z < 0 || z >= P.nb[2])) continue;
      const int q2 = per2 ? floor_div(z, P.nb[2]) : 0;
      for (int y = bi[1] - P.m[1]; y <= bi[1] + P.m[1]; ++y) {
        if (!per1 && (y < 0 || y >= P.nb[1])) continue;
        const int q1 = per1 ? floor_div(y, P.nb[1]) : 0;
        const int64_t row = P.base + ((int64_t)(z - q2 * P.nb[2]) * P.nb[1] +
                                      (y - q1 * P.nb[1])) * P.nb[0];
        int x = bi[0] - P.m[0], x_end = bi[0] + P.m[0];
        if (!per0) {
          x = x < 0 ? 0 : x;
          x_end = x_end >= P.nb[0] ? P.nb[0] - 1 : x_end;
        }
        while (x <= x_end) {  // one image q0 at a time: its bins are consecutive in the table
          const int q0 = per0 ? floor_div(x, P.nb[0]) : 0;
          const int last = (q0 + 1) * P.nb[0] - 1;
          const int seg_end = x_end < last ? x_end : last;
          const int64_t k_beg = crow[row + (x - q0 * P.nb[0])];
          const int64_t k_end = crow[row + (seg_end - q0 * P.nb[0]) + 1];
          for (int64_t k0 = k_beg; k0 < k_end; k0 += 64) {
            const int64_t k = k0 + lane;
            bool ok = false;
            int64_t key = 0;
            if (k < k_end) {
              const int64_t j = cperm[k];
              const int wj = wrap[j];
              const int s0 = q0 - ((wj & 255) - 128) + wi0;
              const int s1 = q1 - (((wj >> 8) & 255) - 128) + wi1;
              const int s2 = q2 - (((wj >> 16) & 255) - 128) + wi2;
              const bool same = !batch || batch[j] == batch[i];  // bins are per graph already
              const bool self = j == i && s0 == 0 && s1 == 0 && s2 == 0;
              ok = same && !self && within(pi, pos, j, cell, s0, s1, s2, r2);
              if (ok && (abs(s0) > 127 || abs(s1) > 127 || abs(s2) > 127)) {
                *err = 1;  // does not pack: the host refuses such inputs before the launch
                ok = false;
              }
              key = (j << 24) | ((int64_t)(s0 + 128) << 16) | ((int64_t)(s1 + 128) << 8) |
                    (int64_t)(s2 + 128);
            }
            const uint64_t mask = __ballot(ok);
            if (MODE) {
              const int64_t slot = filled + __popcll(mask & below);
              if (ok && slot < deg) keys[slot] = key;
            }
            filled += __popcll(mask);
          }
          x = seg_end + 1;
        }
      }
    }
    if (!MODE) {
      if (lane == 0) counts[i] = filled;
      continue;
    }
    if (filled != deg) {  // counts and fill disagree (inputs changed in between): report
      if (lane == 0) *err = 1;
      if (in_lds)
        for (int64_t a = lane; a < deg; a += 64) emit_edge(0, base + a, src, sidx);
      continue;
    }
    if (!in_lds) continue;  // gmp_radius_pbc_sort_i64 finishes this target
    const int n = (int)deg;
    fence_wave();
    for (int k = 2; (k >> 1) < n; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = lane; 2 * t < n + k; t += 64) bitonic_cmp(keys, n, k, j, t);
        fence_wave();
      }
    }
    for (int a = lane; a < n; a += 64) emit_edge(keys[a], base + a, src, sidx);
    fence_wave();  // the next target reuses the buffer
  }
}

// targets with more than kCap edges: src[offs[i], offs[i+1]) holds their packed keys; one
// block sorts the range in place and unpacks it
__global__ __launch_bounds__(kPT) void pbc_sort_kernel(int64_t N, const int64_t* __restrict__ offs,
                                                       int64_t* __restrict__ src,
                                                       int* __restrict__ sidx) {
  for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
    const int64_t base = offs[i], deg = offs[i + 1] - base;
    if (deg <= kCap) continue;  // uniform over the block
    int64_t* keys = src + base;
    const int n = (int)deg;
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
      for (int j = (int)(k >> 1); j > 0; j >>= 1) {
        for (int64_t t = threadIdx.x; 2 * t < n + k; t += kPT)
          bitonic_cmp(keys, n, (int)k, j, (int)t);
        __syncthreads();
      }
    }
    for (int a = threadIdx.x; a < n; a += kPT) emit_edge(keys[a], base + a, src, sidx);
    __syncthreads();
  }
}

__global__ void shift_vectors_kernel(const int* __restrict__ sidx, const float* __restrict__ cell,
                                     const int64_t* __restrict__ graph, int64_t E, int64_t B,
                                     float* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = graph ? graph[e] : 0;
    const bool bad = b < 0 || b >= B;
    const float* c = cell + 9 * (bad ? 0 : b);
    const float f0 = (float)sidx[3 * e], f1 = (float)sidx[3 * e + 1], f2 = (float)sidx[3 * e + 2];
    for (int k = 0; k < 3; ++k) {
      const float t = add_rn(add_rn(mul_rn(f0, c[k]), mul_rn(f1, c[3 + k])), mul_rn(f2, c[6 + k]));
      out[3 * e + k] = bad ? 0.f : t;
    }
  }
}

int grid_for(int64_t n, int per_block) {
  int64_t g = ceil_div(n, per_block);
  const int64_t cap = (int64_t)device_cu_count() * 16;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

int scan_launch(int mode, const float* pos, const int64_t* batch, int64_t n_nodes,
                int64_t n_graphs, float r, const int* graph_i, const float* graph_f,
                const int64_t* graph_base, const int64_t* bin, const int* wrap,
                const int64_t* bin_rowptr, const int64_t* bin_perm, int64_t* counts,
                const int64_t* offsets, int64_t* src_out, int* shift_out, int32_t* err_flag,
                void* stream) {
  GMP_CHECK_ARG(n_nodes >= 0 && n_graphs >= 1 && r > 0.f);
  if (n_nodes == 0) return GMP_OK;
  GMP_CHECK_ARG(n_nodes <= INT32_MAX);  // a node id and three shifts pack into one 64-bit key
  GMP_CHECK_ARG(pos && graph_i && graph_f && graph_base && bin && wrap && bin_rowptr &&
                bin_perm && err_flag);
  const float r2 = r * r;
  const int grid = grid_for(n_nodes, kPT / 64);
  if (mode == 0) {
    GMP_CHECK_ARG(counts);
    pbc_scan_kernel<0><<<grid, kPT, 0, as_stream(stream)>>>(
        pos, batch, n_nodes, n_graphs, r2, graph_i, graph_f, graph_base, bin, wrap, bin_rowptr,
        bin_perm, counts, nullptr, nullptr, nullptr, err_flag);
  } else {
    GMP_CHECK_ARG(offsets && src_out && shift_out);
    pbc_scan_kernel<1><<<grid, kPT, 0, as_stream(stream)>>>(
        pos, batch, n_nodes, n_graphs, r2, graph_i, graph_f, graph_base, bin, wrap, bin_rowptr,
        bin_perm, nullptr, offsets, src_out, shift_out, err_flag);
    if (launch_status() != GMP_OK) return GMP_ERR_HIP;
    pbc_sort_kernel<<<grid_for(n_nodes, 1), kPT, 0, as_stream(stream)>>>(n_nodes, offsets,
                                                                         src_out, shift_out);
  }
  return launch_status();
}

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int gmp_radius_pbc_sort_capacity(void) { return kCap; }

int gmp_radius_pbc_bins_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                            int64_t n_graphs, const int* graph_i, const float* graph_f,
                            const int64_t* graph_base, int64_t* bin_out, int* wrap_out,
                            int32_t* err_flag, void* stream) {
  GMP_CHECK_ARG(n_nodes >= 0 && n_graphs >= 1);
  if (n_nodes == 0) return GMP_OK;
  GMP_CHECK_ARG(pos && graph_i && graph_f && graph_base && bin_out && wrap_out && err_flag);
  pbc_bin_kernel<<<grid_for(n_nodes, 256), 256, 0, as_stream(stream)>>>(
      pos, batch, n_nodes, n_graphs, graph_i, graph_f, graph_base, bin_out, wrap_out, err_flag);
  return launch_status();
}

int gmp_radius_pbc_count_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                             int64_t n_graphs, float r, const int* graph_i, const float* graph_f,
                             const int64_t* graph_base, const int64_t* bin, const int* wrap,
                             const int64_t* bin_rowptr, const int64_t* bin_perm, int64_t* counts,
                             int32_t* err_flag, void* stream) {
  return scan_launch(0, pos, batch, n_nodes, n_graphs, r, graph_i, graph_f, graph_base, bin, wrap,
                     bin_rowptr, bin_perm, counts, nullptr, nullptr, nullptr, err_flag, stream);
}

int gmp_radius_pbc_fill_f32(const float* pos, const int64_t* batch, int64_t n_nodes,
                            int64_t n_graphs, float r, const int* graph_i, const float* graph_f,
                            const int64_t* graph_base, const int64_t* bin, const int* wrap,
                            const int64_t* bin_rowptr, const int64_t* bin_perm,
                            const int64_t* offsets, int64_t* src_out, int* shift_idx_out,
                            int32_t* err_flag, void* stream) {
  return scan_launch(1, pos, batch, n_nodes, n_graphs, r, graph_i, graph_f, graph_base, bin, wrap,
                     bin_rowptr, bin_perm, nullptr, offsets, src_out, shift_idx_out, err_flag,
                     stream);
}

int gmp_edge_shift_vectors_f32(const int* edge_shift_idx, const float* cell,
                               const int64_t* edge_graph, int64_t n_edges, int64_t n_graphs,
                               float* shift_out, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_graphs >= 1);
  if (n_edges == 0) return GMP_OK;
  GMP_CHECK_ARG(edge_shift_idx && cell && shift_out);
  shift_vectors_kernel<<<grid_for(n_edges, 256), 256, 0, as_stream(stream)>>>(
      edge_shift_idx, cell, edge_graph, n_edges, n_graphs, shift_out);
  return launch_status();
}

}  // extern "C"
