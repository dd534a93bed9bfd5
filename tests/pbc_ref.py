"""Brute-force numpy restatement of the periodic radius-graph contract (include/gmp.h, K9p),
shared by tests/test_pbc_host.py and tests/test_gpu_pbc.py.  Not a test module.

Every (i, j, S) with S up to the reach of the cutoff plus the spread of the atoms' wraps is
tested with the contract's fp32 formula (numpy float32: every operation rounded, nothing
contracted), so the lists are exact, not approximate.  Also here: the periodic oracle models
(the fp64 reference of the model tests) and a few structures both test files use.
"""
import itertools

import numpy as np
import torch

from oracle import mace as omace
from oracle import schnet as osch


def shift_vectors(S, cell):
    """t (E, 3) fp32 = ((S0*c0 + S1*c1) + S2*c2), cell (E, 3, 3) or (3, 3) fp32."""
    S = np.asarray(S, np.float32)
    c = np.asarray(cell, np.float32)
    c = np.broadcast_to(c, (S.shape[0], 3, 3))
    return (S[:, 0:1] * c[:, 0] + S[:, 1:2] * c[:, 1]) + S[:, 2:3] * c[:, 2]


def image_range(pos, cell, pbc, r, extra=0):
    """Per axis, the largest |S_k| to enumerate: the reach ceil(r / h_k) of the cutoff over the
    perpendicular height plus the spread of the atoms' fractional coordinates (+ `extra`)."""
    c = np.asarray(cell, np.float64)
    vol = abs(np.linalg.det(c))
    cross = np.stack([np.cross(c[1], c[2]), np.cross(c[2], c[0]), np.cross(c[0], c[1])])
    h = vol / np.linalg.norm(cross, axis=1)
    frac = np.asarray(pos, np.float64) @ np.linalg.inv(c)
    spread = np.ceil(frac.max(0) - frac.min(0)) if len(frac) else np.zeros(3)
    rng = np.ceil(r / h) + spread + 1 + extra
    return [int(rng[k]) if pbc[k] else 0 for k in range(3)]


def radius_graph_pbc(pos, r, cell, pbc=(True, True, True), batch=None, extra=0):
    """(edge_index (2, E) int64, edge_shift_idx (E, 3) int32) of the contract, sorted by
    (i, j, S0, S1, S2).  pos (N, 3), cell (B, 3, 3) or (3, 3); `extra` more image shells."""
    pos = np.asarray(pos, np.float32)
    cell = np.asarray(cell, np.float32).reshape(-1, 3, 3)
    N = pos.shape[0]
    batch = np.zeros(N, np.int64) if batch is None else np.asarray(batch, np.int64)
    r2 = np.float32(r) * np.float32(r)
    rows = []
    for b in range(cell.shape[0]):
        idx = np.nonzero(batch == b)[0]
        if idx.size == 0:
            continue
        p, c = pos[idx], cell[b]
        rng = image_range(p, c, pbc, float(r), extra)
        d0 = p[:, None, :] - p[None, :, :]  # [i, j] = p_i - p_j
        for S in itertools.product(*[range(-k, k + 1) for k in rng]):
            t = (np.float32(S[0]) * c[0] + np.float32(S[1]) * c[1]) + np.float32(S[2]) * c[2]
            d = d0 - t
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            ok = d2 < r2
            if S == (0, 0, 0):
                np.fill_diagonal(ok, False)
            i, j = np.nonzero(ok)
            if i.size:
                rows.append(np.stack([idx[i], idx[j], np.full(i.size, S[0]),
                                      np.full(i.size, S[1]), np.full(i.size, S[2])], 1))
    if not rows:
        return np.zeros((2, 0), np.int64), np.zeros((0, 3), np.int32)
    a = np.concatenate(rows).astype(np.int64)
    a = a[np.lexsort((a[:, 4], a[:, 3], a[:, 2], a[:, 1], a[:, 0]))]
    return np.stack([a[:, 1], a[:, 0]]), a[:, 2:5].astype(np.int32)


# ------------------------------------------------------------------------------ structures
CUBIC = np.eye(3, dtype=np.float32)
FCC = np.array([[0, .5, .5], [.5, 0, .5], [.5, .5, 0]], np.float32)
TRICLINIC = np.array([[6, 0, 0], [1.5, 5, 0], [-1, 2, 7]], np.float32)
THIN = np.array([[1.6, 0, 0], [0.4, 5.5, 0], [-0.3, 1.1, 6.0]], np.float32)  # thinner than r = 2
KNOWN = [  # (cell, pbc, r, edges) for one atom at the origin
    (CUBIC, (True, True, True), 2.5, 80),
    (FCC, (True, True, True), 0.75, 12),
    (FCC, (True, True, True), 1.05, 18),
    (CUBIC, (True, True, False), 1.5, 8),
]


def random_in_cell(n, cell, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) @ np.asarray(cell, np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------ oracle models
class PeriodicSchNet(osch.SchNetModel):
    """oracle.schnet.SchNetModel.forward restated with the image shift added to the edge
    vector: batch.edge_shift (E, 3), same dtype as pos."""

    def forward(self, batch):
        h = self.embedding(batch.atoms)
        row, col = batch.edge_index
        w = (batch.pos[row] - batch.pos[col] + batch.edge_shift).norm(dim=-1)
        attr = self.distance_expansion(w)
        for inter in self.interactions:
            h = h + inter(h, batch.edge_index, w, attr)
        out = self.pool(h, batch.batch)
        return self.lin2(self.act(self.lin1(out)))


class periodic_edge_features:
    """Context manager: oracle.mace.edge_features (MACE and TFN) with `shift` (E, 3) added to
    the edge vectors."""

    def __init__(self, shift):
        self.shift = shift

    def __enter__(self):
        self.prev = omace.edge_features
        shift = self.shift

        def edge_features(pos, edge_index, radial, max_ell=2):
            vectors = pos[edge_index[0]] - pos[edge_index[1]] + shift
            lengths = torch.linalg.norm(vectors, dim=-1, keepdim=True)
            return omace.o3.spherical_harmonics(vectors, max_ell), radial(lengths)

        omace.edge_features = edge_features
        return self

    def __exit__(self, *exc):
        omace.edge_features = self.prev
        return False


def oracle_energy_forces_stress(model, atoms, pos, cell, edge_index, shift_idx, batch,
                                num_graphs, create_graph=False, mace_like=False):
    """fp64: (E, F, sigma) with sigma = (1 / V) dE / d eps at eps = 0 under the symmetric strain
    pos -> pos + pos @ sym(eps)[batch], cell -> cell + cell @ sym(eps).  pos must require grad."""
    from gmp_amd.graph import Batch
    eps = torch.zeros(num_graphs, 3, 3, dtype=pos.dtype, requires_grad=True)
    sym = 0.5 * (eps + eps.transpose(1, 2))
    p = pos + torch.einsum("nd,ndk->nk", pos, sym[batch])
    c = cell + cell @ sym
    graph = batch[edge_index[1]]
    shift = torch.einsum("ek,ekc->ec", shift_idx.to(pos.dtype), c[graph])
    b = Batch(atoms, p, edge_index, batch, num_graphs=num_graphs, edge_shift=shift)
    if mace_like:
        with periodic_edge_features(shift):
            E = model(b)
    else:
        E = model(b)
    g, ge = torch.autograd.grad(E.sum(), (pos, eps), create_graph=create_graph)
    return E, -g, ge / torch.linalg.det(cell).abs().view(-1, 1, 1)
