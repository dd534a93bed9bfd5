"""Plain-torch restatement of SphereNet's geometry on a periodic graph (the SphereNet part of the
K11p contract in include/gmp.h), in the dtype of its inputs; a helper, not a test module.

* lists from dimenet_pbc_ref.triplets, vectors from dimenet_pbc_ref.edge_vectors;
* u = 0 - vec_e, v = vec[idx_kj[t]], the angle at j, and for every candidate t' of the same edge
  w = vec[idx_kj[t']] and t1(t, t') in the contract's operation order, with torch's own CPU ops
  (torch.cross, (x * y).sum(-1), .norm(-1), .pow(2).sum(-1).sqrt(), atan2) as oracle/triplets.py;
* the torsion is the first minimum over the candidates (identity FLT_MAX, NaN never wins, 0 and
  arg -1 if nothing won); with a given `arg` only that candidate is evaluated, so the result is
  differentiable with the winner held fixed, as the scatter-min's backward routes it.

Dead cases go through torch.where, so that no NaN enters a gradient: an exactly zero plane1 x
plane2 pair (a = b = 0: an exactly collinear triplet or a candidate exactly parallel to u) gives
t1 = 2 pi with zero derivative; |u| = 0 gives NaN (0 / 0), which never wins, with zero derivative;
an exactly zero u x v drops the norm's derivative.
"""
import math

import torch

import dimenet_pbc_ref as dref

BIG = float(torch.finfo(torch.float32).max)


def candidates(idx_ji):
    """The (t, t') pairs: every triplet t with all triplets t' of the same edge, t-major, t' in
    index order (idx_ji is non-decreasing, so an edge's triplets are one contiguous range)."""
    T = idx_ji.numel()
    if T == 0:
        z = torch.zeros(0, dtype=torch.long)
        return z, z.clone()
    assert bool((idx_ji[1:] >= idx_ji[:-1]).all())
    n_e = int(idx_ji.max()) + 1
    cnt = torch.bincount(idx_ji, minlength=n_e)
    first = torch.cumsum(cnt, 0) - cnt
    n_c = cnt[idx_ji]
    t_of = torch.repeat_interleave(torch.arange(T), n_c)
    start = torch.cumsum(n_c, 0) - n_c
    c_of = first[idx_ji][t_of] + torch.arange(t_of.numel()) - start[t_of]
    return t_of, c_of


def _t1(u, v, w):
    """t1 of the contract for rows of (u, v, w), and the mask of its dead cases."""
    cross = torch.linalg.cross
    plane1, plane2 = cross(u, v), cross(u, w)
    a = (plane1 * plane2).sum(-1)
    c = (cross(plane1, plane2) * u).sum(-1)
    L = u.pow(2).sum(-1).sqrt()
    one = torch.ones_like(L)
    b = c / torch.where(L == 0, one, L)
    dead = ((a == 0) & (b == 0)) | (L == 0)
    t1 = torch.atan2(torch.where(dead, one, b), torch.where(dead, one, a))
    t1 = torch.where(t1 <= 0, t1 + 2 * math.pi, t1)
    t1 = torch.where(dead, torch.full_like(t1, 2 * math.pi), t1)  # atan2(0, 0) = 0 -> 2 pi
    return torch.where(L == 0, torch.full_like(t1, float("nan")), t1), dead  # 0 / 0: never wins


def _uv(vec, idx_kj, idx_ji):
    return torch.zeros_like(vec)[idx_ji] - vec[idx_ji], vec[idx_kj]


def torsion_candidates(vec, idx_kj, idx_ji):
    """-> t_of, c_of, t1 (per pair, in the contract's operation order)."""
    t_of, c_of = candidates(idx_ji)
    u, v = _uv(vec, idx_kj, idx_ji)
    t1, _ = _t1(u[t_of], v[t_of], vec[idx_kj[c_of]])
    return t_of, c_of, t1


def first_minimum(t_of, c_of, t1, T):
    """-> torsion (T), arg (T): the minimum of t1 per triplet and the candidate (a triplet index)
    that attains it first; identity FLT_MAX, NaN never wins, 0 / -1 if nothing won."""
    v = torch.nan_to_num(t1.detach(), nan=BIG)
    mn = torch.full((T,), BIG, dtype=v.dtype).scatter_reduce(0, t_of, v, "amin", include_self=True)
    none = torch.iinfo(torch.long).max
    cand = torch.where(v == mn[t_of], c_of, torch.full_like(c_of, none))
    arg = torch.full((T,), none).scatter_reduce(0, t_of, cand, "amin", include_self=True)
    won = (mn < BIG) & (arg < none)
    return torch.where(won, mn, torch.zeros_like(mn)), torch.where(won, arg, -torch.ones_like(arg))


def geometry_from_vec(vec, idx_kj, idx_ji, arg=None):
    """-> dist (E), angle (T, vertex j), torsion (T), arg (T).  arg None: the first minimum over
    the candidates, selected on detached values (torsion then carries no gradient).  A given arg
    (triplet indices, -1: none) evaluates that candidate only: differentiable, winner fixed."""
    dist = vec.pow(2).sum(-1).sqrt()
    u, v = _uv(vec, idx_kj, idx_ji)
    angle = torch.atan2(dref._norm_or_zero(torch.linalg.cross(u, v)), (u * v).sum(-1))
    T = idx_kj.numel()
    if arg is None:
        t_of, c_of, t1 = torsion_candidates(vec.detach(), idx_kj, idx_ji)
        torsion, arg = first_minimum(t_of, c_of, t1, T)
        return dist, angle, torsion, arg
    has = arg >= 0
    w = vec[idx_kj[torch.where(has, arg, torch.zeros_like(arg))]]
    t1, _ = _t1(u, v, w)
    return dist, angle, torch.where(has, t1, torch.zeros_like(t1)), arg


def geometry(pos, cell, edge_index, shift_idx, batch=None, arg=None):
    """dist, angle, torsion, i, j, idx_kj, idx_ji, arg of the periodic graph, in the layout of
    xyz_to_dat(use_torsion=True) and in the contract's order."""
    idx_kj, idx_ji = dref.triplets(edge_index, shift_idx)
    vec = dref.edge_vectors(pos, cell, edge_index, shift_idx, batch)
    dist, angle, torsion, arg = geometry_from_vec(vec, idx_kj, idx_ji, arg)
    return dist, angle, torsion, edge_index[1], edge_index[0], idx_kj, idx_ji, arg


def zero_planes(vec, idx_kj, idx_ji):
    """(pairs) bool: plane1 or plane2 exactly zero in vec's dtype, with the pair lists."""
    t_of, c_of = candidates(idx_ji)
    u, v = _uv(vec, idx_kj, idx_ji)
    cross = torch.linalg.cross
    p1 = (cross(u[t_of], v[t_of]) == 0).all(-1)
    p2 = (cross(u[t_of], vec[idx_kj[c_of]]) == 0).all(-1)
    return t_of, c_of, p1 | p2
