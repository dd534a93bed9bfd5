"""Plain-torch restatement of K11p, DimeNet's triplet geometry on a periodic graph (the contract
of include/gmp.h next to K11), in the dtype of its inputs; a helper, not a test module.

* `geometry`: brute-force image-aware triplets in the contract's order, dist and angle from the
  per-edge vectors; differentiable by autograd in pos and cell.
* `vec_bwd` / `vec_bwd2`: closed forms of what gmp_triplet_vec_bwd_f32 and
  gmp_triplet_vec_bwd2_f32 (with the per-edge sums) evaluate, in the style of
  tests/dimenet_bwd2_ref.py.  tests/test_dimenet_pbc_host.py pins them in fp64 to double autograd
  of `geometry`, and pins `geometry` + dimenet_ref.model to an explicit open-boundary cluster of
  images that the unmodified dimenet_ref.geometry enumerates.

An exactly collinear triplet (b = |u x v| = 0; a self-image edge followed by the same self-image
edge gives v = 2u) drops the c^ terms, as the kernels, torch autograd of the norm and PyG do.
"""
import numpy as np
import torch


def _z(t, like):
    return torch.zeros_like(like) if t is None else t


def shift_vectors(shift_idx, cell, graph=None):
    """t (E, 3) = ((S0 c0 + S1 c1) + S2 c2) in cell's dtype, cell (3, 3) or (B, 3, 3) with
    graph (E) the graph of each edge: the K9p contract's order of operations."""
    S = shift_idx.to(cell.dtype)
    c = cell.reshape(-1, 3, 3)
    c = c[graph] if graph is not None else c.expand(S.shape[0], 3, 3)
    return (S[:, 0:1] * c[:, 0] + S[:, 1:2] * c[:, 1]) + S[:, 2:3] * c[:, 2]


def edge_vectors(pos, cell, edge_index, shift_idx, batch=None):
    """vec (E, 3) = (pos[j] - pos[i]) + t_e, e = (j -> i) = (edge_index[0][e], edge_index[1][e])."""
    row, col = edge_index
    graph = batch[col] if batch is not None else None
    return (pos[row] - pos[col]) + shift_vectors(shift_idx, cell, graph)


def triplets(edge_index, shift_idx):
    """idx_kj, idx_ji (T) by brute force: for every edge e = (j -> i, S_e), in edge order, all
    edges kj = (k -> j, S_kj) except those with k == i and S_kj == -S_e, in ascending k, then
    ascending edge id."""
    row, col = (t.numpy() for t in edge_index)
    S = shift_idx.numpy().astype(np.int64)
    kj, ji = [], []
    for e in range(row.shape[0]):
        into_j = np.nonzero(col == row[e])[0]
        into_j = into_j[np.lexsort((into_j, row[into_j]))]
        reverse = (row[into_j] == col[e]) & (S[into_j] == -S[e]).all(1)
        keep = into_j[~reverse]
        kj.append(keep)
        ji.append(np.full(keep.shape[0], e, np.int64))
    if not kj:
        z = torch.zeros(0, dtype=torch.long)
        return z, z.clone()
    return (torch.from_numpy(np.concatenate(kj).astype(np.int64)),
            torch.from_numpy(np.concatenate(ji)))


def _norm_or_zero(c):
    """|c| per row; an exactly zero row gives 0 with zero derivatives of every order (b = 0 drops
    the c^ terms), where autograd of .norm() at 0 turns a second backward into 0 / 0."""
    live = (c != 0).any(-1)
    safe = torch.where(live[:, None], c, torch.ones_like(c))
    return torch.where(live, safe.norm(dim=-1), torch.zeros_like(safe[:, 0]))


def geometry_from_vec(vec, idx_kj, idx_ji):
    """dist (E) = |vec|, angle (T) = atan2(|u x v|, u.v) with u = vec_ji, v = u + vec_kj."""
    dist = vec.pow(2).sum(-1).sqrt()
    u = vec[idx_ji]
    v = u + vec[idx_kj]
    a = (u * v).sum(-1)
    b = _norm_or_zero(torch.linalg.cross(u, v))
    return dist, torch.atan2(b, a)


def geometry(pos, cell, edge_index, shift_idx, batch=None):
    """dist (E), angle (T, vertex i), i, j, idx_kj, idx_ji of the periodic graph, in the layout of
    dimenet_ref.geometry and in the contract's order."""
    idx_kj, idx_ji = triplets(edge_index, shift_idx)
    vec = edge_vectors(pos, cell, edge_index, shift_idx, batch)
    dist, angle = geometry_from_vec(vec, idx_kj, idx_ji)
    return dist, angle, edge_index[1], edge_index[0], idx_kj, idx_ji


def collinear(vec, idx_kj, idx_ji):
    """(T) bool: the exactly collinear triplets (b == 0 in vec's dtype)."""
    u = vec[idx_ji]
    return torch.linalg.cross(u, u + vec[idx_kj]).norm(dim=-1) == 0


def _angle_parts(u, v):
    cross = torch.linalg.cross
    c = cross(u, v)
    b, a = c.norm(dim=-1), (u * v).sum(-1)
    live = b > 0
    bs = torch.where(live, b, torch.ones_like(b))
    return c, a, b, live, bs


def vec_bwd(vec, idx_kj, idx_ji, g_dist, g_angle):
    """-> g_vec (E, 3), the gradient of sum(g_dist dist) + sum(g_angle angle) w.r.t. vec."""
    cross = torch.linalg.cross
    E, T = vec.shape[0], idx_kj.numel()
    g_dist = _z(g_dist, vec.new_zeros(E))
    g_angle = _z(g_angle, vec.new_zeros(T))
    ln = vec.pow(2).sum(-1).sqrt()
    g_vec = (g_dist / ln)[:, None] * vec
    u = vec[idx_ji]
    v = u + vec[idx_kj]
    c, a, b, live, bs = _angle_parts(u, v)
    den = a * a + b * b
    ga, gb = -g_angle * b / den, g_angle * a / den
    ch = live[:, None].to(vec.dtype) * c / bs[:, None]
    gu = ga[:, None] * v + gb[:, None] * cross(v, ch)
    gv = ga[:, None] * u + gb[:, None] * cross(ch, u)
    return g_vec.index_add(0, idx_ji, gu + gv).index_add(0, idx_kj, gv)


def vec_bwd2(vec, idx_kj, idx_ji, g_dist, g_angle, a_vec):
    """The second backward: with the cotangent a_vec (E, 3) of vec_bwd's g_vec
    -> gg_dist (E), gg_angle (T), h_vec (E, 3)."""
    cross = torch.linalg.cross
    E, T = vec.shape[0], idx_kj.numel()
    g_dist = _z(g_dist, vec.new_zeros(E))
    g_angle = _z(g_angle, vec.new_zeros(T))
    ln = vec.pow(2).sum(-1).sqrt()
    gg_dist = (vec * a_vec).sum(-1) / ln
    h_vec = g_dist[:, None] * (a_vec / ln[:, None] - vec * (gg_dist / ln ** 2)[:, None])
    u, du = vec[idx_ji], a_vec[idx_ji]
    v, dv = u + vec[idx_kj], du + a_vec[idx_kj]
    c, a, b, live, bs = _angle_parts(u, v)
    dc = cross(du, v) + cross(u, dv)
    da = (du * v).sum(-1) + (u * dv).sum(-1)
    db = torch.where(live, (c * dc).sum(-1) / bs, torch.zeros_like(b))
    den = a * a + b * b
    dden = 2 * (a * da + b * db)
    gg_angle = (a * db - b * da) / den
    ga, gb = -g_angle * b / den, g_angle * a / den
    dga = -g_angle * (db / den - b * dden / den ** 2)
    dgb = g_angle * (da / den - a * dden / den ** 2)
    lv = live[:, None].to(vec.dtype)
    ch = lv * c / bs[:, None]
    dch = lv * (dc / bs[:, None] - c * (db / bs ** 2)[:, None])
    col = lambda t: t[:, None]  # noqa: E731
    hu = (col(dga) * v + col(ga) * dv + col(dgb) * cross(v, ch)
          + col(gb) * (cross(dv, ch) + cross(v, dch)))
    hv = (col(dga) * u + col(ga) * du + col(dgb) * cross(ch, u)
          + col(gb) * (cross(dch, u) + cross(ch, du)))
    h_vec = h_vec.index_add(0, idx_ji, hu + hv).index_add(0, idx_kj, hv)
    return gg_dist, gg_angle, h_vec
