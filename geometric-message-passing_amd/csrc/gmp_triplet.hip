// K11: triplet enumeration + angle / torsion featurisation (the "angles"
// of the north star's featurisation list).  Follows models/layers/spherenet_layer.py:496-564
// (`xyz_to_dat`) and the DimeNet forward models/dimenet.py:77-90:
//   edge e = (j -> i); its triplets are the in-edges kj = (k -> j) of j with k != i, in
//   ascending k (the row-major order of torch_sparse's adj_t = SparseTensor(row=i, col=j));
//   triplets of all edges are concatenated in edge order.
//   angle (SphereNet, vertex j): atan2(|(p_i - p_j) x (p_k - p_j)|, (p_i - p_j).(p_k - p_j))
//   angle (DimeNet,   vertex i): atan2(|(p_j - p_i) x (p_k - p_i)|, (p_j - p_i).(p_k - p_i))
//   torsion (SphereNet): min over the in-neighbours k_n != i of j of atan2(b, a) mapped to
//   (0, 2*pi], with plane1 = v_ji x v_jk, plane2 = v_ji x v_jkn, a = plane1.plane2,
//   b = (plane1 x plane2).v_ji / |v_ji|.
// The arithmetic is gmp_triplet_geom.h's, each rounding stated there.  It follows the reference's
// torch CPU evaluation: torch.cross is a_i*b_j - a_j*b_i contracted to fma(a_i, b_j, -(a_j*b_i));
// `(x*y).sum(-1)` rounds each product then adds (((+0 + 0) + 1) + 2); `.norm(-1)` accumulates
// fma(x, x, acc).  This matters beyond the last ulp: for k_n = k plane1 == plane2, and the sign of
// the contracted cross product's rounding residual decides whether that candidate's torsion is
// ~1e-9 or 2*pi — the reference's output depends on it, so the kernel follows it.  The two
// `.pow(2).sum(-1).sqrt()` lengths depart from torch's products, ((0 + 1) + 2), sqrt: dist is
// sqrt(fma(y, y, x x) + z z) and the torsion's |v_ji| is sqrt(fma(x, x, y y) + z z).
#include "gmp_triplet_geom.h"

namespace gmp {
namespace {

__global__ void triplet_count_kernel(const float* __restrict__ pos,
                                     const int64_t* __restrict__ ei, int64_t E,
                                     const int64_t* __restrict__ arow,
                                     const int64_t* __restrict__ asrc,
                                     int64_t* __restrict__ counts, float* __restrict__ dist) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += stride) {
    const int64_t j = ei[e], i = ei[E + e];
    const int64_t r0 = arow[j], r1 = arow[j + 1];
    int64_t p, q;
    equal_range(asrc, r0, r1, i, p, q);
    counts[e] = (r1 - r0) - (q - p);
    if (dist) dist[e] = dist_len3(sub3(ld3(pos, i), ld3(pos, j)));
  }
}

// One workgroup per block of kFB consecutive edges.  Phase 1: a thread per edge puts the
// edge's triplet offset, endpoints and adjacency window (row start, the [p, q) run of source i)
// into LDS.  Phase 2: the block's triplets are spread over all threads; each finds its edge by
// a binary search in LDS (no global-memory search per triplet).
// mode 0: SphereNet angle at j (+ optional torsion); mode 1: DimeNet angle at i
constexpr int kFB = 256;

__global__ __launch_bounds__(kFB) void triplet_fill_kernel(
    const float* __restrict__ pos, const int64_t* __restrict__ ei, int64_t E,
    const int64_t* __restrict__ arow, const int64_t* __restrict__ asrc,
    const int64_t* __restrict__ aeid, const int64_t* __restrict__ offs, int mode,
    int64_t* __restrict__ idx_kj, int64_t* __restrict__ idx_ji, float* __restrict__ angle,
    float* __restrict__ torsion, int64_t* __restrict__ torsion_kn) {
  __shared__ int64_t s_off[kFB + 1];
  __shared__ int64_t s_i[kFB], s_j[kFB], s_r0[kFB], s_r1[kFB], s_p[kFB], s_q[kFB];
  const int64_t e0 = (int64_t)blockIdx.x * kFB;
  const int nE = (int)(E - e0 < kFB ? E - e0 : kFB);
  const int tid = threadIdx.x;
  if (tid < nE) {
    const int64_t e = e0 + tid;
    const int64_t j = ei[e], i = ei[E + e];
    const int64_t r0 = arow[j], r1 = arow[j + 1];
    int64_t p, q;
    equal_range(asrc, r0, r1, i, p, q);
    s_off[tid] = offs[e];
    s_i[tid] = i;
    s_j[tid] = j;
    s_r0[tid] = r0;
    s_r1[tid] = r1;
    s_p[tid] = p;
    s_q[tid] = q;
  }
  if (tid == 0) s_off[nE] = offs[e0 + nE];
  __syncthreads();
  const int64_t t_begin = s_off[0], t_end = s_off[nE];
  for (int64_t t = t_begin + tid; t < t_end; t += kFB) {
    const int lo = find_local_edge(s_off, nE, t);
    const int64_t e = e0 + lo;
    const int64_t i = s_i[lo], j = s_j[lo], r0 = s_r0[lo], r1 = s_r1[lo];
    const int64_t p = s_p[lo], q = s_q[lo];
    const int64_t local = t - s_off[lo];
    const int64_t slot = r0 + local + (r0 + local >= p ? q - p : 0);
    const int64_t k = asrc[slot];
    idx_kj[t] = aeid[slot];
    idx_ji[t] = e;
    if (!angle && !torsion) continue;
    const V3 pi = ld3(pos, i), pj = ld3(pos, j), pk = ld3(pos, k);
    if (angle) {
      V3 u, v;
      if (mode == 0) {
        u = sub3(pi, pj);
        v = sub3(pk, pj);
      } else {
        u = sub3(pj, pi);
        v = sub3(pk, pi);
      }
      angle[t] = atan2f(norm3(cross3(u, v)), dot3_sum(u, v));
    }
    if (torsion) {
      const V3 vji = sub3(pi, pj);
      const float dji = torsion_len3(vji);
      const V3 plane1 = cross3(vji, sub3(pk, pj));
      float best = kNoTorsion;
      int64_t arg = -1;  // the winning candidate k_n (first among equal minima)
      for (int64_t m = r0; m < r1; ++m) {
        const int64_t kn = asrc[m];
        if (kn == i) continue;
        const float t1 = torsion_candidate(vji, plane1, dji, sub3(ld3(pos, kn), pj));
        if (t1 < best) {
          best = t1;
          arg = kn;
        }
      }
      torsion[t] = best == kNoTorsion ? 0.f : best;
      if (torsion_kn) torsion_kn[t] = arg;
    }
  }
}

// Backward of dist and angle w.r.t. pos (dimenet.py:82-89 / spherenet_layer.py:509,531-535
// under autograd).  theta = atan2(b, a), a = u.v, b = |c|, c = u x v:
//   d theta = (a db - b da) / (a^2 + b^2);  da/du = v, da/dv = u;
//   db/du = v x c^, db/dv = c^ x u (c^ = c / b; 0 when b = 0, as torch's norm backward).
// Rows written (3 floats each): [0, T) vertex -(g_u + g_v), [T, 2T) u end g_u, [2T, 3T) v end
// g_v, [3T, 3T+E) g_d (p_i - p_j) / d at i, [3T+E, 3T+2E) its negative at j; node[] receives
// the row's node so one segmented sum over a CSR of node[] yields d pos deterministically.
__global__ void triplet_geom_bwd_kernel(const float* __restrict__ pos,
                                        const int64_t* __restrict__ ei, int64_t E,
                                        const int64_t* __restrict__ idx_kj,
                                        const int64_t* __restrict__ idx_ji, int64_t T, int mode,
                                        const float* __restrict__ g_dist,
                                        const float* __restrict__ g_angle,
                                        float* __restrict__ rows, int64_t* __restrict__ node) {
  const int64_t n = T + E;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    if (q < T) {
      const int64_t t = q, e = idx_ji[t];
      const int64_t j = ei[e], i = ei[E + e], k = ei[idx_kj[t]];
      const int64_t vtx = mode == 0 ? j : i, ue = mode == 0 ? i : j;
      const V3 pv = ld3(pos, vtx), u = sub3(ld3(pos, ue), pv), v = sub3(ld3(pos, k), pv);
      V3 gu, gv;
      angle_bwd(u, v, g_angle ? g_angle[t] : 0.f, gu, gv);
      st3(rows + 3 * t, neg3(acc3(gu, gv)));
      st3(rows + 3 * (T + t), gu);
      st3(rows + 3 * (2 * T + t), gv);
      node[t] = vtx;
      node[T + t] = ue;
      node[2 * T + t] = k;
    } else {
      const int64_t e = q - T;
      const int64_t j = ei[e], i = ei[E + e];
      dist_bwd_row(sub3(ld3(pos, i), ld3(pos, j)), g_dist ? g_dist[e] : 0.f,
                   rows + 3 * (3 * T + e), rows + 3 * (3 * T + E + e));
      node[3 * T + e] = i;
      node[3 * T + E + e] = j;
    }
  }
}

// Second backward of dist and angle (energy-and-force training, dimenet.py:82-89 differentiated
// twice): the first backward's rows are linear in (g_dist, g_angle) and non-linear in pos; with
// the cotangent a (N, 3) of d pos this kernel returns
//   gg_dist[e]  = (a_i - a_j).(p_i - p_j) / d,   gg_angle[t] = a_u.dtheta/du + a_v.dtheta/dv
//   (a_u = a[ue] - a[vtx], a_v = a[k] - a[vtx]), and
//   rows: the directional derivative along (a_u, a_v) / (a_i - a_j) of the rows that
//   triplet_geom_bwd_kernel writes (= g Hess(theta) (a_u, a_v), g Hess(d) (a_i - a_j)), in the
//   same layout with the same node[], so the same segmented sum yields h_pos.
// Forward mode (value + tangent) of the formulas above; the differences are taken in fp32 as
// there, the rest runs in double and is rounded once (second derivatives divide by b^2, d^2).
// Dead cases as the first backward: b = 0 drops the c^ terms and their tangents, len = 0 and
// g == 0 write zero rows (gg_* is still written).
__global__ void triplet_geom_bwd2_kernel(const float* __restrict__ pos,
                                         const int64_t* __restrict__ ei, int64_t E,
                                         const int64_t* __restrict__ idx_kj,
                                         const int64_t* __restrict__ idx_ji, int64_t T, int mode,
                                         const float* __restrict__ g_dist,
                                         const float* __restrict__ g_angle,
                                         const float* __restrict__ a_pos,
                                         float* __restrict__ gg_dist,
                                         float* __restrict__ gg_angle, float* __restrict__ rows,
                                         int64_t* __restrict__ node) {
  const int64_t n = T + E;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    if (q < T) {
      const int64_t t = q, e = idx_ji[t];
      const int64_t j = ei[e], i = ei[E + e], k = ei[idx_kj[t]];
      const int64_t vtx = mode == 0 ? j : i, ue = mode == 0 ? i : j;
      const V3 pv = ld3(pos, vtx), av = ld3(a_pos, vtx);
      const D3 u = dd3(sub3(ld3(pos, ue), pv)), v = dd3(sub3(ld3(pos, k), pv));
      const D3 du = dd3(sub3(ld3(a_pos, ue), av)), dv = dd3(sub3(ld3(a_pos, k), av));
      const double g = g_angle ? (double)g_angle[t] : 0.0;
      D3 hu, hv;
      const double gg = angle_bwd2(u, v, du, dv, g, hu, hv);
      if (gg_angle) gg_angle[t] = (float)gg;
      st3(rows + 3 * t, dscale(-1.0, dadd(hu, hv)));
      st3(rows + 3 * (T + t), hu);
      st3(rows + 3 * (2 * T + t), hv);
      node[t] = vtx;
      node[T + t] = ue;
      node[2 * T + t] = k;
    } else {
      const int64_t e = q - T;
      const int64_t j = ei[e], i = ei[E + e];
      const D3 d = dd3(sub3(ld3(pos, i), ld3(pos, j)));
      const D3 dd = dd3(sub3(ld3(a_pos, i), ld3(a_pos, j)));
      D3 h;
      const double dlen = dist_bwd2(d, dd, g_dist ? (double)g_dist[e] : 0.0, h);
      if (gg_dist) gg_dist[e] = (float)dlen;
      st3(rows + 3 * (3 * T + e), h);
      st3(rows + 3 * (3 * T + E + e), dscale(-1.0, h));
      node[3 * T + e] = i;
      node[3 * T + E + e] = j;
    }
  }
}

// Backward of the SphereNet torsion w.r.t. pos (spherenet_layer.py:535-559 under autograd): the
// scatter-min routes the gradient to the winning candidate k_n (torch_scatter's arg), whose
// torsion1 = atan2(b, a) is differentiated by torsion_bwd with u = p_i - p_j, v = p_k - p_j,
// w = p_kn - p_j.  Rows [0, T) at i (gu), [T, 2T) at j (-(gu + gv + gw)), [2T, 3T) at k (gv),
// [3T, 4T) at k_n (gw); triplets without a candidate (k_n < 0) and torsion_bwd's dead cases (an
// edge of zero length, an exactly collinear triplet or winner) write zero rows.
__global__ void triplet_torsion_bwd_kernel(const float* __restrict__ pos,
                                           const int64_t* __restrict__ ei, int64_t E,
                                           const int64_t* __restrict__ idx_kj,
                                           const int64_t* __restrict__ idx_ji,
                                           const int64_t* __restrict__ kn_of, int64_t T,
                                           const float* __restrict__ g_tor,
                                           float* __restrict__ rows, int64_t* __restrict__ node) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = idx_ji[t];
    const int64_t j = ei[e], i = ei[E + e], k = ei[idx_kj[t]], kn = kn_of[t];
    const float g = g_tor[t];
    V3 gu{0.f, 0.f, 0.f}, gv{0.f, 0.f, 0.f}, gw{0.f, 0.f, 0.f};
    if (kn >= 0) {
      const V3 pj = ld3(pos, j);
      torsion_bwd(sub3(ld3(pos, i), pj), sub3(ld3(pos, k), pj), sub3(ld3(pos, kn), pj), g, gu,
                  gv, gw);
    }
    st3(rows + 3 * t, gu);
    st3(rows + 3 * (T + t), neg3(acc3(acc3(gu, gv), gw)));
    st3(rows + 3 * (2 * T + t), gv);
    st3(rows + 3 * (3 * T + t), gw);
    node[t] = i;
    node[T + t] = j;
    node[2 * T + t] = k;
    node[3 * T + t] = kn >= 0 ? kn : i;
  }
}

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int gmp_triplet_count(const float* pos, const int64_t* edge_index, int64_t n_edges,
                      int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                      int64_t* counts, float* dist, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_nodes >= 0);
  if (n_edges == 0) return GMP_OK;
  GMP_CHECK_ARG(edge_index && adj_rowptr && adj_src && counts && (pos || !dist));
  triplet_count_kernel<<<triplet_grid_for(n_edges), 256, 0, as_stream(stream)>>>(
      pos, edge_index, n_edges, adj_rowptr, adj_src, counts, dist);
  return launch_status();
}

int gmp_triplet_fill_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                         int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                         const int64_t* adj_eid, const int64_t* offsets, int64_t n_triplets,
                         int mode, int64_t* idx_kj, int64_t* idx_ji, float* angle,
                         float* torsion, int64_t* torsion_kn, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_nodes >= 0 && n_triplets >= 0 && (mode == 0 || mode == 1));
  GMP_CHECK_ARG(mode == 0 || !torsion);
  GMP_CHECK_ARG(!torsion_kn || torsion);
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(n_edges > 0 && edge_index && adj_rowptr && adj_src && adj_eid && offsets &&
                idx_kj && idx_ji && (pos || (!angle && !torsion)));
  triplet_fill_kernel<<<(unsigned)ceil_div(n_edges, kFB), kFB, 0, as_stream(stream)>>>(
      pos, edge_index, n_edges, adj_rowptr, adj_src, adj_eid, offsets, mode, idx_kj, idx_ji,
      angle, torsion, torsion_kn);
  return launch_status();
}

int gmp_triplet_geom_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                             const int64_t* idx_kj, const int64_t* idx_ji, int64_t n_triplets,
                             int mode, const float* grad_dist, const float* grad_angle,
                             float* rows, int64_t* node, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0 && (mode == 0 || mode == 1));
  if (n_edges + n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(pos && edge_index && rows && node && (n_triplets == 0 || (idx_kj && idx_ji)));
  triplet_geom_bwd_kernel<<<triplet_grid_for(n_edges + n_triplets), 256, 0, as_stream(stream)>>>(
      pos, edge_index, n_edges, idx_kj, idx_ji, n_triplets, mode, grad_dist, grad_angle, rows,
      node);
  return launch_status();
}

int gmp_triplet_geom_bwd2_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                              const int64_t* idx_kj, const int64_t* idx_ji, int64_t n_triplets,
                              int mode, const float* grad_dist, const float* grad_angle,
                              const float* a_pos, float* gg_dist, float* gg_angle, float* rows,
                              int64_t* node, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0 && (mode == 0 || mode == 1));
  if (n_edges + n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(pos && a_pos && edge_index && rows && node &&
                (n_triplets == 0 || (idx_kj && idx_ji)));
  triplet_geom_bwd2_kernel<<<triplet_grid_for(n_edges + n_triplets), 256, 0, as_stream(stream)>>>(
      pos, edge_index, n_edges, idx_kj, idx_ji, n_triplets, mode, grad_dist, grad_angle, a_pos,
      gg_dist, gg_angle, rows, node);
  return launch_status();
}

int gmp_triplet_torsion_bwd_f32(const float* pos, const int64_t* edge_index, int64_t n_edges,
                                const int64_t* idx_kj, const int64_t* idx_ji,
                                const int64_t* torsion_kn, int64_t n_triplets,
                                const float* grad_torsion, float* rows, int64_t* node,
                                void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0);
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(pos && edge_index && idx_kj && idx_ji && torsion_kn && grad_torsion && rows &&
                node);
  triplet_torsion_bwd_kernel<<<triplet_grid_for(n_triplets), 256, 0, as_stream(stream)>>>(
      pos, edge_index, n_edges, idx_kj, idx_ji, torsion_kn, n_triplets, grad_torsion, rows, node);
  return launch_status();
}

}  // extern "C"
