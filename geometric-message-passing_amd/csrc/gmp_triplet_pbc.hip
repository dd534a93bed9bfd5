// K11p: DimeNet's triplets and angles on a periodic graph (the contract is stated in
// include/gmp.h next to K11).  An edge is e = (j -> i, S_e) with the K9p vector
// vec_e = (pos[j] - pos[i]) + t_e; its triplets are the entries kj = (k -> j, S_kj) of j's
// in-adjacency except the reverse images of e (k == i and S_kj == -S_e, an integer compare);
//   dist[e] = dist_len3(vec_e),  angle[t] = atan2(|u x v|, u.v),  u = vec_ji, v = u + vec_kj
// (v: the image of k relative to i).  The geometry is a function of the per-edge vectors only,
// so the backward kernels work in edge-vector form: they take vec (E, 3) and write per-triplet
// and per-edge rows that are summed per edge over CSRs the model already holds (no node[] array,
// no sort per backward); pos and cell are reached through the linear maps vec = P pos + t.
// The per-triplet arithmetic is gmp_triplet_geom.h's, shared with the node-form kernels.
#include "gmp_triplet_geom.h"

namespace gmp {
namespace {

struct I3 {
  int x, y, z;
};
__device__ __forceinline__ I3 ldi3(const int32_t* __restrict__ p, int64_t a) {
  return I3{p[3 * a], p[3 * a + 1], p[3 * a + 2]};
}
// the entry's shift is the negative of s (s of the edge whose reverse image is excluded)
__device__ __forceinline__ bool is_neg(I3 a, I3 s) {
  return a.x == -s.x && a.y == -s.y && a.z == -s.z;
}

// counts[e] = in-degree(j) - #{entries (i -> j, -S_e)}: equal_range on source i, then a scan of
// that run (the images of i around j: short) for the reverse images.
__global__ void triplet_count_pbc_kernel(const float* __restrict__ vec,
                                         const int64_t* __restrict__ ei, int64_t E,
                                         const int64_t* __restrict__ arow,
                                         const int64_t* __restrict__ asrc,
                                         const int64_t* __restrict__ aeid,
                                         const int32_t* __restrict__ sidx,
                                         int64_t* __restrict__ counts,
                                         float* __restrict__ dist) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += stride) {
    const int64_t j = ei[e], i = ei[E + e];
    const int64_t r0 = arow[j], r1 = arow[j + 1];
    int64_t p, q;
    equal_range(asrc, r0, r1, i, p, q);
    const I3 s = ldi3(sidx, e);
    int64_t excluded = 0;
    for (int64_t m = p; m < q; ++m) excluded += is_neg(ldi3(sidx, aeid[m]), s) ? 1 : 0;
    counts[e] = (r1 - r0) - excluded;
    if (dist) dist[e] = dist_len3(ld3(vec, e));
  }
}

// The two phases of triplet_fill_kernel (a workgroup per block of kFBp edges: the edge windows
// staged in LDS, then the block's triplets spread over the threads).  The excluded entries are
// no longer one contiguous run: a triplet whose slot falls at or after the start p of the run of
// source i walks the run and skips the reverse images; past the run nothing is excluded.
constexpr int kFBp = 256;

__global__ __launch_bounds__(kFBp) void triplet_fill_pbc_kernel(
    const float* __restrict__ vec, const int64_t* __restrict__ ei, int64_t E,
    const int64_t* __restrict__ arow, const int64_t* __restrict__ asrc,
    const int64_t* __restrict__ aeid, const int32_t* __restrict__ sidx,
    const int64_t* __restrict__ offs, int64_t* __restrict__ idx_kj,
    int64_t* __restrict__ idx_ji, float* __restrict__ angle) {
  __shared__ int64_t s_off[kFBp + 1];
  __shared__ int64_t s_r0[kFBp], s_r1[kFBp], s_p[kFBp], s_q[kFBp];
  __shared__ int s_sx[kFBp], s_sy[kFBp], s_sz[kFBp];
  const int64_t e0 = (int64_t)blockIdx.x * kFBp;
  const int nE = (int)(E - e0 < kFBp ? E - e0 : kFBp);
  const int tid = threadIdx.x;
  if (tid < nE) {
    const int64_t e = e0 + tid;
    const int64_t j = ei[e], i = ei[E + e];
    const int64_t r0 = arow[j], r1 = arow[j + 1];
    int64_t p, q;
    equal_range(asrc, r0, r1, i, p, q);
    const I3 s = ldi3(sidx, e);
    s_off[tid] = offs[e];
    s_r0[tid] = r0;
    s_r1[tid] = r1;
    s_p[tid] = p;
    s_q[tid] = q;
    s_sx[tid] = s.x;
    s_sy[tid] = s.y;
    s_sz[tid] = s.z;
  }
  if (tid == 0) s_off[nE] = offs[e0 + nE];
  __syncthreads();
  const int64_t t_begin = s_off[0], t_end = s_off[nE];
  for (int64_t t = t_begin + tid; t < t_end; t += kFBp) {
    const int lo = find_local_edge(s_off, nE, t);
    const int64_t e = e0 + lo;
    const int64_t r0 = s_r0[lo], r1 = s_r1[lo], p = s_p[lo], q = s_q[lo];
    int64_t slot = r0 + (t - s_off[lo]);
    if (slot >= p) {
      const I3 s{s_sx[lo], s_sy[lo], s_sz[lo]};
      int64_t rem = slot - p, m = p;  // the rem-th kept entry at or after p
      for (; m < q; ++m) {
        if (is_neg(ldi3(sidx, aeid[m]), s)) continue;
        if (rem == 0) break;
        --rem;
      }
      slot = m + rem;
    }
    if (slot >= r1) slot = r1 > r0 ? r1 - 1 : 0;  // offsets that disagree with the count
    const int64_t kj = aeid[slot];
    idx_kj[t] = kj;
    idx_ji[t] = e;
    if (angle) {
      const V3 u = ld3(vec, e), v = add3(u, ld3(vec, kj));
      angle[t] = atan2f(norm3(cross3(u, v)), dot3_sum(u, v));
    }
  }
}

// First backward in edge-vector form.  rows (2T + E, 3): [0, T) g_u + g_v, the share of edge
// idx_ji[t] (u and v both carry vec_ji); [T, 2T) g_v, the share of edge idx_kj[t];
// [2T, 2T + E) g_dist vec / d.  The caller sums [0, T) over the triplet offsets, [T, 2T) over the
// CSR of idx_kj and adds [2T, 2T + E): deterministic, no atomics.
__global__ void triplet_vec_bwd_kernel(const float* __restrict__ vec, int64_t E,
                                       const int64_t* __restrict__ idx_kj,
                                       const int64_t* __restrict__ idx_ji, int64_t T,
                                       const float* __restrict__ g_dist,
                                       const float* __restrict__ g_angle,
                                       float* __restrict__ rows) {
  const int64_t n = T + E;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    if (q < T) {
      const int64_t t = q;
      const V3 u = ld3(vec, idx_ji[t]), v = add3(u, ld3(vec, idx_kj[t]));
      V3 gu, gv;
      angle_bwd(u, v, g_angle ? g_angle[t] : 0.f, gu, gv);
      st3(rows + 3 * t, acc3(gu, gv));
      st3(rows + 3 * (T + t), gv);
    } else {
      const int64_t e = q - T;
      dist_bwd_row(ld3(vec, e), g_dist ? g_dist[e] : 0.f, rows + 3 * (2 * T + e));
    }
  }
}

// Second backward in edge-vector form: with the cotangent a_vec (E, 3) of the first backward's
// g_vec, a_u = a_vec[ji] and a_v = a_vec[ji] + a_vec[kj] (fp32, as u and v),
//   gg_dist[e] = a_vec_e . vec_e / d,  gg_angle[t] = a_u.dtheta/du + a_v.dtheta/dv,
//   rows: the directional derivative along a_vec of the rows triplet_vec_bwd_kernel writes, in
//   its layout.  Conventions of triplet_geom_bwd2_kernel: everything after u, v, a_u, a_v in
//   double, rounded once; the dead cases of the first backward.
__global__ void triplet_vec_bwd2_kernel(const float* __restrict__ vec, int64_t E,
                                        const int64_t* __restrict__ idx_kj,
                                        const int64_t* __restrict__ idx_ji, int64_t T,
                                        const float* __restrict__ g_dist,
                                        const float* __restrict__ g_angle,
                                        const float* __restrict__ a_vec,
                                        float* __restrict__ gg_dist,
                                        float* __restrict__ gg_angle,
                                        float* __restrict__ rows) {
  const int64_t n = T + E;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    if (q < T) {
      const int64_t t = q, ji = idx_ji[t], kj = idx_kj[t];
      const V3 u32 = ld3(vec, ji), a32 = ld3(a_vec, ji);
      const D3 u = dd3(u32), v = dd3(add3(u32, ld3(vec, kj)));
      const D3 du = dd3(a32), dv = dd3(add3(a32, ld3(a_vec, kj)));
      const double g = g_angle ? (double)g_angle[t] : 0.0;
      D3 hu, hv;
      const double gg = angle_bwd2(u, v, du, dv, g, hu, hv);
      if (gg_angle) gg_angle[t] = (float)gg;
      st3(rows + 3 * t, dadd(hu, hv));
      st3(rows + 3 * (T + t), hv);
    } else {
      const int64_t e = q - T;
      const D3 d = dd3(ld3(vec, e)), dd = dd3(ld3(a_vec, e));
      D3 h;
      const double dlen = dist_bwd2(d, dd, g_dist ? (double)g_dist[e] : 0.0, h);
      if (gg_dist) gg_dist[e] = (float)dlen;
      st3(rows + 3 * (2 * T + e), h);
    }
  }
}

// ------------------------------------------------------------------------------------------
// SphereNet's angle and torsion on the lists above (the K11p contract, "SphereNet" part): for
// triplet t of edge e, u = 0 - vec_e, v = vec[idx_kj[t]], angle at j; the torsion is the minimum
// over the triplets t' of the same edge (w = vec[idx_kj[t']]) of atan2(b, a) mapped to (0, 2 pi].
// With zero shifts this is triplet_fill_kernel's mode 0 bit for bit: both call the same helpers
// of gmp_triplet_geom.h, whose roundings are explicit.
//
// A thread per triplet; it walks the candidate range [offs[e], offs[e+1]) of its edge (K11's
// form).  plane2 is recomputed per pair: 9 of the ~110 VALU operations of a pair, the rest is
// the division and atan2f.
__global__ void triplet_dat_pbc_kernel(const float* __restrict__ vec,
                                       const int64_t* __restrict__ idx_kj,
                                       const int64_t* __restrict__ idx_ji,
                                       const int64_t* __restrict__ offs, int64_t T,
                                       float* __restrict__ angle, float* __restrict__ torsion,
                                       int64_t* __restrict__ torsion_arg) {
  const V3 zero{0.f, 0.f, 0.f};
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < T;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = idx_ji[t];
    const V3 u = sub3(zero, ld3(vec, e)), v = ld3(vec, idx_kj[t]);
    const V3 plane1 = cross3(u, v);
    if (angle) angle[t] = atan2f(norm3(plane1), dot3_sum(u, v));
    if (!torsion) continue;
    const float dji = torsion_len3(u);
    float best = kNoTorsion;
    int64_t arg = -1;  // first among equal minima
    const int64_t o1 = offs[e + 1];
    for (int64_t c = offs[e]; c < o1; ++c) {
      const float t1 = torsion_candidate(u, plane1, dji, ld3(vec, idx_kj[c]));
      if (t1 < best) {
        best = t1;
        arg = c;
      }
    }
    torsion[t] = best == kNoTorsion ? 0.f : best;
    torsion_arg[t] = arg;
  }
}

// First backward of dist, angle and torsion in edge-vector form.  rows (2T + E, 3) in the layout
// of triplet_vec_bwd_kernel: [0, T) -g_u, the share of edge idx_ji[t] (u = -vec_e); [T, 2T) the
// share of edge idx_kj[t]: g_v of the triplet's own angle and torsion, plus g_w of every triplet
// of the same edge whose winner is t (gathered by walking the edge's range in index order:
// integer compares, a fixed order, no atomics); [2T, 2T + E) g_dist vec / d.  A winner outside
// the edge's range (-1: none) gives the torsion no rows.
__global__ void triplet_dat_vec_bwd_kernel(const float* __restrict__ vec, int64_t E,
                                           const int64_t* __restrict__ idx_kj,
                                           const int64_t* __restrict__ idx_ji,
                                           const int64_t* __restrict__ offs,
                                           const int64_t* __restrict__ targ, int64_t T,
                                           const float* __restrict__ g_dist,
                                           const float* __restrict__ g_angle,
                                           const float* __restrict__ g_tor,
                                           float* __restrict__ rows) {
  const int64_t n = T + E;
  const V3 zero{0.f, 0.f, 0.f};
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n;
       q += (int64_t)gridDim.x * blockDim.x) {
    if (q < T) {
      const int64_t t = q, e = idx_ji[t];
      const V3 u = sub3(zero, ld3(vec, e)), v = ld3(vec, idx_kj[t]);
      V3 gu, gv;
      angle_bwd(u, v, g_angle ? g_angle[t] : 0.f, gu, gv);
      if (g_tor) {
        const int64_t o0 = offs[e], o1 = offs[e + 1], arg = targ[t];
        V3 tu, tv, tw;
        if (arg >= o0 && arg < o1) {
          torsion_bwd(u, v, ld3(vec, idx_kj[arg]), g_tor[t], tu, tv, tw);
          gu = acc3(gu, tu);
          gv = acc3(gv, tv);
        }
        for (int64_t c = o0; c < o1; ++c) {
          if (targ[c] != t) continue;
          torsion_bwd(u, ld3(vec, idx_kj[c]), v, g_tor[c], tu, tv, tw);
          gv = acc3(gv, tw);
        }
      }
      st3(rows + 3 * t, neg3(gu));
      st3(rows + 3 * (T + t), gv);
    } else {
      const int64_t e = q - T;
      dist_bwd_row(ld3(vec, e), g_dist ? g_dist[e] : 0.f, rows + 3 * (2 * T + e));
    }
  }
}

}  // namespace
}  // namespace gmp

using namespace gmp;

extern "C" {

int gmp_triplet_dat_pbc_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                            const int64_t* idx_ji, const int64_t* offsets, int64_t n_triplets,
                            float* angle, float* torsion, int64_t* torsion_arg, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0);
  GMP_CHECK_ARG((torsion == nullptr) == (torsion_arg == nullptr));
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(n_edges > 0 && vec && idx_kj && idx_ji && (angle || torsion) &&
                (offsets || !torsion));
  triplet_dat_pbc_kernel<<<triplet_grid_for(n_triplets), 256, 0, as_stream(stream)>>>(
      vec, idx_kj, idx_ji, offsets, n_triplets, angle, torsion, torsion_arg);
  return launch_status();
}

int gmp_triplet_dat_vec_bwd_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                                const int64_t* idx_ji, const int64_t* offsets,
                                const int64_t* torsion_arg, int64_t n_triplets,
                                const float* grad_dist, const float* grad_angle,
                                const float* grad_torsion, float* rows, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0);
  if (n_edges + n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(n_edges > 0 && vec && rows && (n_triplets == 0 || (idx_kj && idx_ji)));
  GMP_CHECK_ARG(n_triplets == 0 || !grad_torsion || (offsets && torsion_arg));
  triplet_dat_vec_bwd_kernel<<<triplet_grid_for(n_edges + n_triplets), 256, 0,
                               as_stream(stream)>>>(vec, n_edges, idx_kj, idx_ji, offsets,
                                                    torsion_arg, n_triplets, grad_dist,
                                                    grad_angle, grad_torsion, rows);
  return launch_status();
}

int gmp_triplet_count_pbc(const float* vec, const int64_t* edge_index, int64_t n_edges,
                          int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                          const int64_t* adj_eid, const int32_t* shift_idx, int64_t* counts,
                          float* dist, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_nodes >= 0);
  if (n_edges == 0) return GMP_OK;
  GMP_CHECK_ARG(edge_index && adj_rowptr && adj_src && adj_eid && shift_idx && counts &&
                (vec || !dist));
  triplet_count_pbc_kernel<<<triplet_grid_for(n_edges), 256, 0, as_stream(stream)>>>(
      vec, edge_index, n_edges, adj_rowptr, adj_src, adj_eid, shift_idx, counts, dist);
  return launch_status();
}

int gmp_triplet_fill_pbc_f32(const float* vec, const int64_t* edge_index, int64_t n_edges,
                             int64_t n_nodes, const int64_t* adj_rowptr, const int64_t* adj_src,
                             const int64_t* adj_eid, const int32_t* shift_idx,
                             const int64_t* offsets, int64_t n_triplets, int64_t* idx_kj,
                             int64_t* idx_ji, float* angle, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_nodes >= 0 && n_triplets >= 0);
  if (n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(n_edges > 0 && edge_index && adj_rowptr && adj_src && adj_eid && shift_idx &&
                offsets && idx_kj && idx_ji && (vec || !angle));
  triplet_fill_pbc_kernel<<<(unsigned)ceil_div(n_edges, kFBp), kFBp, 0, as_stream(stream)>>>(
      vec, edge_index, n_edges, adj_rowptr, adj_src, adj_eid, shift_idx, offsets, idx_kj,
      idx_ji, angle);
  return launch_status();
}

int gmp_triplet_vec_bwd_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                            const int64_t* idx_ji, int64_t n_triplets, const float* grad_dist,
                            const float* grad_angle, float* rows, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0);
  if (n_edges + n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(n_edges > 0 && vec && rows && (n_triplets == 0 || (idx_kj && idx_ji)));
  triplet_vec_bwd_kernel<<<triplet_grid_for(n_edges + n_triplets), 256, 0,
                           as_stream(stream)>>>(vec, n_edges, idx_kj, idx_ji, n_triplets,
                                                grad_dist, grad_angle, rows);
  return launch_status();
}

int gmp_triplet_vec_bwd2_f32(const float* vec, int64_t n_edges, const int64_t* idx_kj,
                             const int64_t* idx_ji, int64_t n_triplets, const float* grad_dist,
                             const float* grad_angle, const float* a_vec, float* gg_dist,
                             float* gg_angle, float* rows, void* stream) {
  GMP_CHECK_ARG(n_edges >= 0 && n_triplets >= 0);
  if (n_edges + n_triplets == 0) return GMP_OK;
  GMP_CHECK_ARG(n_edges > 0 && vec && a_vec && rows && (n_triplets == 0 || (idx_kj && idx_ji)));
  triplet_vec_bwd2_kernel<<<triplet_grid_for(n_edges + n_triplets), 256, 0,
                            as_stream(stream)>>>(vec, n_edges, idx_kj, idx_ji, n_triplets,
                                                 grad_dist, grad_angle, a_vec, gg_dist,
                                                 gg_angle, rows);
  return launch_status();
}

}  // extern "C"
