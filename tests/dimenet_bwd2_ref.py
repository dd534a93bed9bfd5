"""Closed forms of the second backwards of DimeNet++'s three non-linear stages (a helper, not a
test module), in plain torch and in the dtype of their inputs: what the kernels
gmp_triplet_geom_bwd2_f32, gmp_dime_edge_basis_bwd2_f32 and gmp_dime_triplet_proj_bwd2_f32
evaluate.  tests/test_dimenet_forces_host.py pins each of them in fp64 to double autograd of
tests/dimenet_ref.py; the GPU tests compare the kernels against them.

Notation: a first backward maps cotangents g_* to gradients; the second backward receives the
cotangents a_* of those gradients and returns gg_* (w.r.t. the g_*) and h_* (w.r.t. the primal
inputs).  An absent (None) cotangent counts as zero.
"""
import math

import torch

import spherenet_ref as sref
from gmp_amd.spherenet import basis_tables


def _z(t, like):
    return torch.zeros_like(like) if t is None else t


# ------------------------------------------------------------------------------- 1. geometry
def geom_bwd2(pos, edge_index, idx_kj, idx_ji, mode, g_dist, g_angle, a_pos):
    """-> gg_dist (E), gg_angle (T), h_pos (N, 3).  mode 0: angle at vertex j (SphereNet), mode 1:
    at vertex i (DimeNet); edge e = (j -> i) = (edge_index[0][e], edge_index[1][e]).  A collinear
    triplet (b = 0) drops the c^ terms, as the first backward does."""
    row, col = edge_index
    E, T = row.numel(), idx_kj.numel()
    g_dist = _z(g_dist, pos.new_zeros(E))
    g_angle = _z(g_angle, pos.new_zeros(T))
    h_pos = torch.zeros_like(pos)
    # distances
    d, dd = pos[col] - pos[row], a_pos[col] - a_pos[row]
    ln = d.pow(2).sum(-1).sqrt()
    gg_dist = (d * dd).sum(-1) / ln
    h_e = g_dist[:, None] * (dd / ln[:, None] - d * (gg_dist / ln ** 2)[:, None])
    h_pos = h_pos.index_add(0, col, h_e).index_add(0, row, -h_e)
    # angles
    e = idx_ji
    jj, ii, kk = row[e], col[e], row[idx_kj]
    vtx, ue = (jj, ii) if mode == 0 else (ii, jj)
    u, v = pos[ue] - pos[vtx], pos[kk] - pos[vtx]
    du, dv = a_pos[ue] - a_pos[vtx], a_pos[kk] - a_pos[vtx]
    cross = torch.linalg.cross
    c, dc = cross(u, v), cross(du, v) + cross(u, dv)
    b, a = c.norm(dim=-1), (u * v).sum(-1)
    live = b > 0
    bs = torch.where(live, b, torch.ones_like(b))
    da = (du * v).sum(-1) + (u * dv).sum(-1)
    db = torch.where(live, (c * dc).sum(-1) / bs, torch.zeros_like(b))
    den = a * a + b * b
    dden = 2 * (a * da + b * db)
    gg_angle = (a * db - b * da) / den
    ga, gb = -g_angle * b / den, g_angle * a / den
    dga = -g_angle * (db / den - b * dden / den ** 2)
    dgb = g_angle * (da / den - a * dden / den ** 2)
    lv = live[:, None].to(pos.dtype)
    ch = lv * c / bs[:, None]
    dch = lv * (dc / bs[:, None] - c * (db / bs ** 2)[:, None])
    col_ = lambda t: t[:, None]  # noqa: E731
    hu = (col_(dga) * v + col_(ga) * dv + col_(dgb) * cross(v, ch)
          + col_(gb) * (cross(dv, ch) + cross(v, dch)))
    hv = (col_(dga) * u + col_(ga) * du + col_(dgb) * cross(ch, u)
          + col_(gb) * (cross(dch, u) + cross(ch, du)))
    h_pos = h_pos.index_add(0, ue, hu).index_add(0, kk, hv).index_add(0, vtx, -(hu + hv))
    return gg_dist, gg_angle, h_pos


# ------------------------------------------------------------------------------- 2. edge basis
def envelope012(x, exponent):
    """The envelope and its first two derivatives; a power with coefficient zero is skipped."""
    p = exponent + 1
    a, b, c = -(p + 1) * (p + 2) / 2, p * (p + 2), -p * (p + 1) / 2

    def pw(q):
        return x ** q if q >= 0 else torch.zeros_like(x)

    v = 1.0 / x + a * pw(p - 1) + b * pw(p) + c * pw(p + 1)
    d1 = -1.0 / x ** 2 + a * (p - 1) * pw(p - 2) + b * p * pw(p - 1) + c * (p + 1) * pw(p)
    d2 = (2.0 / x ** 3 + a * (p - 1) * (p - 2) * pw(p - 3) + b * p * (p - 1) * pw(p - 2)
          + c * (p + 1) * p * pw(p - 1))
    return v, d1, d2


def bessel012(l, y):
    """j_l, j_l', j_l'' at y > 0."""
    j = sref.sph_jl(l, y)
    dj = -sref.sph_jl(1, y) if l == 0 else sref.sph_jl(l - 1, y) - (l + 1) / y * j
    d2j = -(2.0 / y) * dj - (1.0 - l * (l + 1) / y ** 2) * j
    return j, dj, d2j


def edge_basis_bwd2(dist, freq, n, k, cutoff, exponent, g_rbf, g_sbe, a_dist, a_freq):
    """-> gg_rbf (E, k), gg_sbe (E, n k), h_dist (E), h_freq (k); exact zeros for d >= cutoff."""
    E, dt = dist.numel(), dist.dtype
    zeros, norm, _ = basis_tables(n, k)
    z = torch.from_numpy(zeros).to(dt).reshape(1, n * k)
    N = torch.from_numpy(norm).to(dt).reshape(1, n * k)
    g_rbf = _z(g_rbf, dist.new_zeros(E, k))
    g_sbe = _z(g_sbe, dist.new_zeros(E, n * k))
    ad = _z(a_dist, dist.new_zeros(E))[:, None]
    af = _z(a_freq, dist.new_zeros(k))[None, :]
    xr = (dist / cutoff)[:, None]
    live = xr < 1.0
    x = torch.where(live, xr, torch.full_like(xr, 0.5))
    env, d1, d2 = envelope012(x, exponent)
    f = freq[None, :]
    s, c = torch.sin(f * x), torch.cos(f * x)
    m = d1 * x * c + env * c - env * f * x * s
    gg_rbf = ad * (d1 * s + env * f * c) / cutoff + af * env * x * c
    h_dist = (ad * g_rbf * (d2 * s + 2 * d1 * f * c - env * f * f * s)).sum(1) / cutoff ** 2 \
        + (af * g_rbf * m).sum(1) / cutoff
    h_freq_rows = g_rbf * (ad * m / cutoff - af * env * x * x * s)
    J = [bessel012(l, z[:, l * k:(l + 1) * k] * x) for l in range(n)]
    j, dj, d2j = (torch.cat([t[i] for t in J], 1) for i in range(3))
    gg_sbe = ad * N * (d1 * j + env * z * dj) / cutoff
    h_dist = h_dist + (ad * g_sbe * N * (d2 * j + 2 * d1 * z * dj + env * z * z * d2j)).sum(1) \
        / cutoff ** 2
    lv = live.to(dt)
    return gg_rbf * lv, gg_sbe * lv, h_dist * lv[:, 0], (h_freq_rows * lv).sum(0)


# ------------------------------------------------------------------------------- 3. projection
def legendre_y012(n, theta):
    """(T, n) each: Y_l0, dY_l0/dtheta, d2Y_l0/dtheta2 from the Legendre recurrence in
    z = cos(theta): dY = -sin P', d2Y = sin^2 P'' - cos P'."""
    z, s = torch.cos(theta), torch.sin(theta)
    P, D, S = [], [], []
    for l in range(n):
        if l == 0:
            p, d, e = torch.ones_like(z), torch.zeros_like(z), torch.zeros_like(z)
        elif l == 1:
            p, d, e = z, torch.ones_like(z), torch.zeros_like(z)
        else:
            p = ((2 * l - 1) * z * P[-1] - (l - 1) * P[-2]) / l
            d = ((2 * l - 1) * (P[-1] + z * D[-1]) - (l - 1) * D[-2]) / l
            e = ((2 * l - 1) * (2 * D[-1] + z * S[-1]) - (l - 1) * S[-2]) / l
        P.append(p), D.append(d), S.append(e)
    pref = [math.sqrt((2 * l + 1) / (4 * math.pi)) for l in range(n)]
    Y = torch.stack([pref[l] * P[l] for l in range(n)], 1)
    Y1 = torch.stack([-pref[l] * s * D[l] for l in range(n)], 1)
    Y2 = torch.stack([pref[l] * (s * s * S[l] - z * D[l]) for l in range(n)], 1)
    return Y, Y1, Y2


def proj_bwd2(sbe, angle, idx_kj, n, k, W, gS, a_sbe, a_angle, a_W):
    """W, a_W (L, b, n k) (a_W may be None), gS (L, T, b) -> gg_S (L, T, b), h_W (L, b, n k),
    h_sbe (E, n k) (the per-triplet rows summed per edge), h_angle (T)."""
    T = angle.numel()
    Y, Y1, Y2 = (t.repeat_interleave(k, dim=1) for t in legendre_y012(n, angle))
    s = sbe[idx_kj]
    asb = _z(a_sbe, sbe)[idx_kj]
    aa = _z(a_angle, angle)[:, None]
    aW = _z(a_W, W)
    sbf = s * Y
    sdot = asb * Y + s * Y1 * aa
    gg_S = torch.einsum("lbf,tf->ltb", W, sdot) + torch.einsum("lbf,tf->ltb", aW, sbf)
    h_W = torch.einsum("ltb,tf->lbf", gS, sdot)
    u = torch.einsum("lbf,ltb->tf", W, gS)
    udot = torch.einsum("lbf,ltb->tf", aW, gS)
    rows = udot * Y + u * Y1 * aa
    h_sbe = torch.zeros_like(sbe).index_add(0, idx_kj, rows) if T else torch.zeros_like(sbe)
    h_angle = (udot * s * Y1 + u * asb * Y1 + aa * u * s * Y2).sum(1)
    return gg_S, h_W, h_sbe, h_angle
