"""Plain-torch restatement of DimeNet++ (PyG 2.3.1 DimeNetPlusPlus) downstream of the geometry (a
helper, not a test module), in the dtype of its inputs (fp64, or fp32 for the allowance of the
model tests).  Built on spherenet_ref: the edge basis, the envelope, the m = 0 columns of the
harmonics, lin and residual, plus the [x < 1] factor of PyG's envelope; the layers are
index_select / index_add_ compositions.  PyG is not available to the tests, so parity rests on
this restatement; tests/test_dimenet_host.py pins its basis to the golden vectors of the
reference (tests/golden/spherenet.pt).  Everything is differentiable by autograd.
"""
import torch

import spherenet_ref as sref
from spherenet_ref import lin, residual, swish  # noqa: F401
from gmp_amd.spherenet import basis_tables


def envelope(x, exponent=5):
    """PyG's Envelope: the polynomial envelope times [x < 1]."""
    return sref.envelope(x, exponent) * (x < 1.0).to(x.dtype)


def edge_basis(dist, freq, n, k, cutoff, exponent=5):
    """rbf (E, k) = env sin(freq x), sbe (E, n k) = env N_lq j_l(z_lq x)."""
    x = (dist / cutoff).unsqueeze(-1)
    mask = (x < 1.0).to(dist.dtype)
    rbf, jb = sref.edge_basis(dist, freq, n, k, cutoff, exponent)
    if jb.dtype != dist.dtype:  # the tables are fp64
        jb = jb.to(dist.dtype)
    return rbf * mask, jb * (sref.envelope(x, exponent) * mask)


def legendre_y(n, angle):
    """(T, n): Y_l0(angle), the m = 0 columns of the harmonics."""
    Y = sref.harmonics(n, angle, torch.zeros_like(angle))
    return torch.stack([Y[:, l * l] for l in range(n)], 1)


def triplet_embedding(sbe, angle, idx_kj, n, k):
    """sbf (T, n k)[t, l k + q] = sbe[idx_kj[t], l k + q] Y_l0(angle_t)."""
    T = angle.numel()
    return (sbe[idx_kj].view(T, n, k) * legendre_y(n, angle).view(T, n, 1)).reshape(T, n * k)


def bases(dist, angle, idx_kj, freq, n, k, cutoff, exponent=5):
    rbf, sbe = edge_basis(dist, freq, n, k, cutoff, exponent)
    return rbf, triplet_embedding(sbe, angle, idx_kj, n, k)


def interact(xd, S, W, idx_kj, idx_ji, E):
    """gather * product * index_add_: the message of K19d."""
    msg = xd[idx_kj] * (S @ W.t())
    return torch.zeros(E, xd.shape[1], dtype=xd.dtype).index_add_(0, idx_ji, msg)


def interaction(sd, name, x, rbf, sbf, idx_kj, idx_ji, n_skip=(1, 2)):
    x_ji = swish(lin(sd, name + ".lin_ji", x))
    x_kj = swish(lin(sd, name + ".lin_kj", x))
    x_kj = x_kj * lin(sd, name + ".lin_rbf2", lin(sd, name + ".lin_rbf1", rbf))
    x_kj = swish(lin(sd, name + ".lin_down", x_kj))
    m = interact(x_kj, lin(sd, name + ".lin_sbf1", sbf), sd[name + ".lin_sbf2.weight"], idx_kj,
                 idx_ji, x.shape[0])
    h = x_ji + swish(lin(sd, name + ".lin_up", m))
    for r in range(n_skip[0]):
        h = residual(sd, f"{name}.layers_before_skip.{r}", h)
    h = swish(lin(sd, name + ".lin", h)) + x
    for r in range(n_skip[1]):
        h = residual(sd, f"{name}.layers_after_skip.{r}", h)
    return h


def output(sd, name, x, rbf, i, N, n_lins=3):
    x = lin(sd, name + ".lin_rbf", rbf) * x
    v = torch.zeros(N, x.shape[1], dtype=x.dtype).index_add_(0, i, x)
    v = lin(sd, name + ".lin_up", v)
    for r in range(n_lins):
        v = swish(lin(sd, f"{name}.lins.{r}", v))
    return lin(sd, name + ".lin", v)


def model(sd, kw, atoms, dist, angle, i, j, idx_kj, idx_ji, batch, num_graphs):
    """DimeNetPPModel.forward downstream of dimenet_angles for the state_dict `sd` and the
    constructor arguments `kw`."""
    n, k = kw.get("num_spherical", 7), kw.get("num_radial", 6)
    L = kw.get("num_layers", 4)
    rbf, sbf = bases(dist, angle, idx_kj, sd["rbf.freq"], n, k, kw.get("cutoff", 10),
                     kw.get("envelope_exponent", 5))
    N = atoms.shape[0]
    h = sd["emb.emb.weight"][atoms]
    rbf0 = swish(lin(sd, "emb.lin_rbf", rbf))
    x = swish(lin(sd, "emb.lin", torch.cat([h[i], h[j], rbf0], -1)))
    skips = (kw.get("num_before_skip", 1), kw.get("num_after_skip", 2))
    n_lins = kw.get("num_output_layers", 3)
    P = output(sd, "output_blocks.0", x, rbf, i, N, n_lins)
    for l in range(L):
        x = interaction(sd, f"interaction_blocks.{l}", x, rbf, sbf, idx_kj, idx_ji, skips)
        P = P + output(sd, f"output_blocks.{l + 1}", x, rbf, i, N, n_lins)
    return torch.zeros(num_graphs, P.shape[1], dtype=P.dtype).index_add_(0, batch, P)


def geometry(pos, edge_index):
    """dist (E), angle (T, vertex i), i, j, idx_kj, idx_ji from pos (N, 3) and edge_index (2, E)
    as models/dimenet.py:79-90 forms them; the triplets of edge e = (j -> i) are the edges
    (k -> j), k != i, in ascending edge order, grouped by e (PyG's DimeNet.triplets up to the
    order within an edge, which no sum here depends on beyond rounding)."""
    row, col = edge_index  # j, i
    E = row.numel()
    kj, ji = [], []
    for e in range(E):
        into_j = ((col == row[e]) & (row != col[e])).nonzero().flatten()
        kj.append(into_j)
        ji.append(torch.full_like(into_j, e))
    idx_kj = torch.cat(kj) if kj else torch.zeros(0, dtype=torch.long)
    idx_ji = torch.cat(ji) if ji else torch.zeros(0, dtype=torch.long)
    i, j = col, row
    dist = (pos[i] - pos[j]).pow(2).sum(-1).sqrt()
    idx_i, idx_j, idx_k = col[idx_ji], row[idx_ji], row[idx_kj]
    pos_ji, pos_ki = pos[idx_j] - pos[idx_i], pos[idx_k] - pos[idx_i]
    a = (pos_ji * pos_ki).sum(-1)
    b = torch.linalg.cross(pos_ji, pos_ki).norm(dim=-1)
    return dist, torch.atan2(b, a), i, j, idx_kj, idx_ji
