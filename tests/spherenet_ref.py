"""Plain-torch fp64 restatement of SphereNet downstream of the geometry (a helper, not a test
module): the bases from their formulas, the layers as index_select / index_add_ compositions.

Written from the formulas: j_l by series / recurrence, the real harmonics from the standard
associated Legendre functions (Condon-Shortley phase, sin^m theta inside P_l^m) with cos(m phi) /
sin(m phi).  tests/test_spherenet_host.py pins it to the golden fp64 vectors of the reference to
1e-10, so GPU tests on shapes the golden does not hold rest on the reference through it.
Everything is differentiable by autograd.
"""
import math

import torch

from gmp_amd.spherenet import basis_tables


def swish(x):
    return x * torch.sigmoid(x)


def sph_jl(l, x):
    """j_l(x), x (…) fp64 > 0."""
    pre = torch.ones_like(x)
    for i in range(1, l + 1):
        pre = pre * x / (2 * i + 1)
    h = -0.5 * x * x
    term, total = torch.ones_like(x), torch.ones_like(x)
    for k in range(1, 41):
        term = term * h / (k * (2 * l + 2 * k + 1))
        total = total + term
    series = pre * total
    xs = torch.where(x < l + 1, torch.full_like(x, float(l + 1)), x)  # keeps the unused lane tame
    j0 = torch.sin(xs) / xs
    j1 = (j0 - torch.cos(xs)) / xs
    if l == 0:
        rec = j0
    else:
        for i in range(1, l):
            j0, j1 = j1, (2 * i + 1) / xs * j1 - j0
        rec = j1
    return torch.where(x < l + 1, series, rec)


def harmonics(n, theta, phi):
    """(T, n^2): per l the order m = 0, 1..l (cos), -l..-1 (sin)."""
    z, s = torch.cos(theta), torch.sin(theta)
    P = {}
    for m in range(n):
        pmm = torch.ones_like(z)
        for i in range(1, m + 1):
            pmm = pmm * (-(2 * i - 1)) * s
        P[(m, m)] = pmm
        if m + 1 < n:
            P[(m + 1, m)] = (2 * m + 1) * z * pmm
        for l in range(m + 2, n):
            P[(l, m)] = ((2 * l - 1) * z * P[(l - 1, m)] - (l + m - 1) * P[(l - 2, m)]) / (l - m)
    cols = []
    for l in range(n):
        def pref(m):
            return math.sqrt((2 * l + 1) * math.factorial(l - m)
                             / (4 * math.pi * math.factorial(l + m)))
        cols.append(pref(0) * P[(l, 0)])
        for m in range(1, l + 1):
            cols.append(math.sqrt(2.0) * pref(m) * P[(l, m)] * torch.cos(m * phi))
        for m in range(l, 0, -1):
            cols.append(math.sqrt(2.0) * pref(m) * P[(l, m)] * torch.sin(m * phi))
    return torch.stack(cols, 1)


def envelope(x, exponent):
    p = exponent + 1
    a, b, c = -(p + 1) * (p + 2) / 2, p * (p + 2), -p * (p + 1) / 2
    return 1.0 / x + a * x ** (p - 1) + b * x ** p + c * x ** (p + 1)


def edge_basis(dist, freq, n, k, cutoff, exponent=5):
    """rbf (E, k), jb (E, n k) in fp64."""
    zeros, norm, _ = basis_tables(n, k)
    x = (dist / cutoff).unsqueeze(-1)
    rbf = envelope(x, exponent) * torch.sin(freq * x)
    zt = torch.from_numpy(zeros).double()
    nt = torch.from_numpy(norm).double()
    jb = torch.stack([nt[l] * sph_jl(l, zt[l] * x) for l in range(n)], 1)
    return rbf, jb.reshape(dist.numel(), n * k)


def triplet_embeddings(jb, angle, torsion, idx_kj, n, k):
    """angle_emb (T, n k), torsion_emb (T, n^2 k) in the reference's layout."""
    Y = harmonics(n, angle, torsion)
    T = angle.numel()
    g = jb[idx_kj].view(T, n, k)
    y0 = torch.stack([Y[:, l * l] for l in range(n)], 1)
    a = (g * y0.view(T, n, 1)).reshape(T, n * k)
    t = (g.view(T, 1, n, k) * Y.view(T, n, n, 1)).reshape(T, n * n * k)
    return a, t


def embeddings(dist, angle, torsion, idx_kj, freq, n, k, cutoff, exponent=5):
    rbf, jb = edge_basis(dist, freq, n, k, cutoff, exponent)
    a, t = triplet_embeddings(jb, angle, torsion, idx_kj, n, k)
    return rbf, a, t


def lin(sd, name, x):
    y = x @ sd[name + ".weight"].t()
    return y + sd[name + ".bias"] if name + ".bias" in sd else y


def residual(sd, name, x):
    return x + swish(lin(sd, name + ".lin2", swish(lin(sd, name + ".lin1", x))))


def interact(xd, S, P, Wa, Wt, idx_kj, idx_ji, E):
    """gather * product * index_add_: the message of K19."""
    msg = xd[idx_kj] * (S @ Wa.t()) * (P @ Wt.t())
    return torch.zeros(E, xd.shape[1], dtype=xd.dtype).index_add_(0, idx_ji, msg)


def update_e(sd, name, x1, rbf0, sbf, t, idx_kj, idx_ji, n_skip=(1, 2)):
    x_ji = swish(lin(sd, name + ".lin_ji", x1))
    x_kj = swish(lin(sd, name + ".lin_kj", x1))
    x_kj = x_kj * lin(sd, name + ".lin_rbf2", lin(sd, name + ".lin_rbf1", rbf0))
    x_kj = swish(lin(sd, name + ".lin_down", x_kj))
    m = interact(x_kj, lin(sd, name + ".lin_sbf1", sbf), lin(sd, name + ".lin_t1", t),
                 sd[name + ".lin_sbf2.weight"], sd[name + ".lin_t2.weight"], idx_kj, idx_ji,
                 x1.shape[0])
    e1 = x_ji + swish(lin(sd, name + ".lin_up", m))
    for r in range(n_skip[0]):
        e1 = residual(sd, f"{name}.layers_before_skip.{r}", e1)
    e1 = swish(lin(sd, name + ".lin", e1)) + x1
    for r in range(n_skip[1]):
        e1 = residual(sd, f"{name}.layers_after_skip.{r}", e1)
    return e1, lin(sd, name + ".lin_rbf", rbf0) * e1


def model(sd, kw, cutoff, atoms, dist, angle, torsion, i, j, idx_kj, idx_ji, batch, num_graphs):
    """SphereNetModel.forward downstream of xyz_to_dat for the state_dict `sd` (fp64) and the
    constructor arguments `kw`; only the branches that reach the output are evaluated."""
    n, k = kw.get("num_spherical", 7), kw.get("num_radial", 6)
    L = kw.get("num_layers", 4)
    rbf, sbf, t = embeddings(dist, angle, torsion, idx_kj, sd["emb.dist_emb.freq"], n, k, cutoff,
                             kw.get("envelope_exponent", 5))
    N = atoms.shape[0]
    if kw.get("use_node_features", True):
        x = sd["init_e.emb.weight"][atoms]
    else:
        x = sd["init_e.node_embedding"][None, :].expand(N, -1)
    rbf0 = swish(lin(sd, "init_e.lin_rbf_0", rbf))
    e1 = swish(lin(sd, "init_e.lin", torch.cat([x[i], x[j], rbf0], -1)))
    skips = (kw.get("num_before_skip", 1), kw.get("num_after_skip", 2))
    e2 = None
    for l in range(L):
        e1, e2 = update_e(sd, f"update_es.{l}", e1, rbf, sbf, t, idx_kj, idx_ji, skips)
    name = f"update_vs.{L - 1}"
    v = torch.zeros(N, e2.shape[1], dtype=e2.dtype).index_add_(0, i, e2)
    v = lin(sd, name + ".lin_up", v)
    for r in range(kw.get("num_output_layers", 2)):
        v = swish(lin(sd, f"{name}.lins.{r}", v))
    v = lin(sd, name + ".lin", v)
    return torch.zeros(num_graphs, v.shape[1], dtype=v.dtype).index_add_(0, batch, v)
