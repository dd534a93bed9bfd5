"""SphereNet on periodic structures, the CPU side: the plain-torch helper
tests/spherenet_pbc_ref.py is pinned (1) with zero shifts, in fp32, bit for bit to the oracle's
xyz_to_dat(use_torsion=True), and (2) in fp64 to an explicit open-boundary cluster of images
whose triplets and torsion candidates the unmodified oracle.triplets enumerates, a path that
shares none of the periodic code; plus the header, the ctypes table, the argument checks that
return before any launch, and the `periodic` flag of the model.  No device work.

The cluster comparison is per candidate and circular (mod 2 pi), not of the minimum: the self
candidate and tie-type candidates sit at 0 = 2 pi, where the sign of a rounding residue decides.  A
pair whose plane1 or plane2 is exactly zero in the periodic helper has no torsion (the helper
gives 2 pi); it is left out of the circular compare, and the share of such pairs is capped.
"""
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import dimenet_pbc_ref as dref
import pbc_ref
import spherenet_pbc_ref as sref
from conftest import ROOT
from oracle import triplets as otri

CELL_1D = np.array([[1.7, 0, 0], [0, 9, 0], [0, 0, 9]], np.float32)
# (name, cell, pbc, atoms, r): the 1-D cell of test_dimenet_pbc_host, and THIN with 12 atoms (its
# 3-atom structure there is mostly self-image edges: 30 % of its pairs have a zero plane)
STRUCTURES = [
    ("1d-thin", CELL_1D, (True, False, False), 4, 2.0),
    ("thin12", pbc_ref.THIN, (True, True, True), 12, 2.0),
]
NEW_SYMBOLS = ("gmp_triplet_dat_pbc_f32", "gmp_triplet_dat_vec_bwd_f32")


def _open_graph(n, box, r, seed):
    """test_gpu_triplets._graph: a shuffled open-boundary radius graph."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 3, generator=g) * box
    d = torch.cdist(pos.double(), pos.double())
    ei = torch.nonzero((d < r) & (d > 0)).T.flip(0).contiguous()
    return pos, ei[:, torch.randperm(ei.shape[1], generator=g)]


@pytest.mark.parametrize("n,box,r", [(60, 4.0, 1.6), (300, 6.0, 1.5)])
def test_zero_shifts_equal_the_oracle_bit_for_bit(n, box, r):
    pos, ei = _open_graph(n, box, r, n)
    E = ei.shape[1]
    S = torch.zeros(E, 3, dtype=torch.long)
    out = sref.geometry(pos, torch.eye(3) * 50, ei, S)
    want = otri.xyz_to_dat(pos, ei, n, use_torsion=True)
    print(f"N {n} E {E} T {want[-1].numel()}")
    assert want[-1].numel() > 1000
    for k, name in enumerate(["dist", "angle", "torsion", "i", "j", "idx_kj", "idx_ji"]):
        assert torch.equal(out[k], want[k]), name
    # the winner is a triplet index of the same edge
    arg, ji = out[7], out[6]
    assert bool((arg >= 0).all()) and torch.equal(ji[arg], ji)


def _structure(name, cell, pbc, n, r):
    if name == "1d-thin":  # keep the atoms within reach of each other across the open axes
        frac = np.random.default_rng(1).random((n, 3))
        frac[:, 1:] = 0.5 + 0.12 * (frac[:, 1:] - 0.5)
        pos = (frac @ cell.astype(np.float64)).astype(np.float32)
    else:
        pos = pbc_ref.random_in_cell(n, cell, 3)
    ei, S = pbc_ref.radius_graph_pbc(pos, r, cell, pbc)
    return pos, torch.from_numpy(ei), torch.from_numpy(S).long()


def _circular(x, y):
    return abs((x - y + math.pi) % (2 * math.pi) - math.pi)


@pytest.mark.parametrize("case", STRUCTURES, ids=[c[0] for c in STRUCTURES])
def test_periodic_helper_equals_explicit_cluster(case):
    name, cell, pbc, n, r = case
    pos, ei, S = _structure(name, cell, pbc, n, r)
    c = torch.from_numpy(cell).double()
    p = torch.from_numpy(pos).double()
    kj, ji = dref.triplets(ei, S)
    vec = dref.edge_vectors(p, c, ei, S)
    _, angle, _, _ = sref.geometry_from_vec(vec, kj, ji)
    t_of, c_of, t1 = sref.torsion_candidates(vec, kj, ji)
    _, _, zero = sref.zero_planes(vec, kj, ji)
    row, col = ei

    # the explicit cluster: every image within 2 r of the cell, the central cell first
    h = pbc_ref.image_range(pos, cell, pbc, 2 * r)
    imgs = sorted(itertools.product(*[range(-k, k + 1) for k in h]), key=lambda s: s != (0, 0, 0))
    P = torch.cat([p + torch.tensor(s, dtype=torch.float64) @ c for s in imgs])
    img_of = [s for s in imgs for _ in range(n)]
    d = (P[:, None] - P[None]).norm(dim=-1)
    src, dst = ((d < r) & ~torch.eye(len(P), dtype=torch.bool)).nonzero(as_tuple=True)
    cei = torch.stack([src, dst])
    M = P.shape[0]
    idx_i, idx_j, idx_k, _, _ = otri.triplets(cei, M)
    central = idx_i < n
    idx_i, idx_j, idx_k = idx_i[central], idx_j[central], idx_k[central]
    rowptr, asrc, _ = otri.adjacency_by_target(cei, M)

    def atom(m):
        return (int(m) % n,) + tuple(img_of[int(m)])

    cross = torch.linalg.cross
    want_angle, want_t1 = {}, {}
    for i_, j_, k_ in zip(idx_i.tolist(), idx_j.tolist(), idx_k.tolist()):
        u, v = P[i_] - P[j_], P[k_] - P[j_]
        key = (i_, atom(j_), atom(k_))
        want_angle[key] = float(torch.atan2(cross(u, v).norm(), (u * v).sum()))
        p1 = cross(u, v)
        for kn in asrc[rowptr[j_]:rowptr[j_ + 1]].tolist():
            if kn == i_:
                continue
            p2 = cross(u, P[kn] - P[j_])
            a = (p1 * p2).sum()
            b = (cross(p1, p2) * u).sum() / u.norm()
            want_t1[key + (atom(kn),)] = float(torch.atan2(b, a))

    def image(e, base=(0, 0, 0)):
        return (int(row[e]),) + tuple(int(b) + int(s) for b, s in zip(base, S[e]))

    keys = []
    for t in range(kj.numel()):
        a_j = image(int(ji[t]))
        keys.append((int(col[ji[t]]), a_j, image(int(kj[t]), a_j[1:])))
    assert len(set(keys)) == len(keys) == len(want_angle)
    worst_a = max(abs(float(angle[t]) - want_angle[keys[t]]) for t in range(len(keys)))
    assert worst_a <= 1e-10, worst_a
    worst_t, left_out = 0.0, 0
    assert t_of.numel() == len(want_t1)
    for q in range(t_of.numel()):
        t, tc = int(t_of[q]), int(c_of[q])
        key = keys[t] + (image(int(kj[tc]), keys[t][1][1:]),)
        if bool(zero[q]):
            assert float(t1[q]) == 2 * math.pi
            left_out += 1
            continue
        worst_t = max(worst_t, _circular(float(t1[q]), want_t1[key]))
    share = left_out / t_of.numel()
    print(f"{name}: T {len(keys)} pairs {t_of.numel()} angle err {worst_a:.1e} "
          f"t1 err {worst_t:.1e} left out {share:.3f}")
    assert worst_t <= 1e-9, worst_t
    assert share <= 0.10, share


def test_fixed_winner_is_differentiable_and_dead_cases_are_finite():
    name, cell, pbc, n, r = STRUCTURES[0]
    pos, ei, S = _structure(name, cell, pbc, n, r)
    c = torch.from_numpy(cell).double()
    p = torch.from_numpy(pos).double().requires_grad_(True)
    out = sref.geometry(p, c, ei, S)
    arg = out[7]
    assert not out[2].requires_grad
    again = sref.geometry(p, c, ei, S, arg=arg)
    assert torch.equal(again[2].detach(), out[2]) and again[2].requires_grad
    _, _, zero = sref.zero_planes(dref.edge_vectors(p.detach(), c, ei, S), out[5], out[6])
    assert int(zero.sum()) > 0  # exactly collinear self-image triplets are present
    (g,) = torch.autograd.grad(again[1].sum() + again[2].sum(), p)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def test_symbols_declared_exported_and_checked():
    from gmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmp.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 6
    # the checks that return before any launch: no triplets is GMP_OK, a torsion without its
    # winner array (or the reverse) and a negative count are refused
    one = 8
    assert lib.gmp_triplet_dat_pbc_f32(None, 0, None, None, None, 0, None, None, None, None) == 0
    assert lib.gmp_triplet_dat_pbc_f32(one, 1, one, one, one, 1, one, one, None, None) != 0
    assert lib.gmp_triplet_dat_pbc_f32(one, 1, one, one, one, 1, one, None, one, None) != 0
    assert lib.gmp_triplet_dat_pbc_f32(None, 1, None, None, None, -1, None, None, None, None) != 0
    assert lib.gmp_triplet_dat_vec_bwd_f32(None, 0, None, None, None, None, 0, None, None, None,
                                           None, None) == 0
    assert lib.gmp_triplet_dat_vec_bwd_f32(None, 2, None, None, None, None, 0, None, None, None,
                                           None, None) != 0
    assert lib.gmp_triplet_dat_vec_bwd_f32(one, 2, one, one, None, None, 3, None, None, one,
                                           one, None) != 0


def _cpu_batch(**extra):
    from gmp_amd.graph import Batch
    pos = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    ei = torch.tensor([[0, 1, 1, 2, 0, 2], [1, 0, 2, 1, 2, 0]])
    return Batch(torch.ones(3, dtype=torch.long), pos, ei, torch.zeros(3, dtype=torch.long),
                 num_graphs=1, edge_shift_idx=torch.zeros(6, 3, dtype=torch.int32), **extra)


def test_periodic_flag():
    import gmp_amd
    from gmp_amd import triplets
    kw = dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16, num_layers=1)
    on = gmp_amd.SphereNetModel(**kw, periodic=True)
    off = gmp_amd.SphereNetModel(**kw)
    assert on.periodic is True and not hasattr(off, "periodic")
    sig = inspect.signature(gmp_amd.SphereNetModel.__init__)
    assert sig.parameters["periodic"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["periodic"].default is False
    # neither a parameter nor a buffer
    assert list(on.state_dict()) == list(off.state_dict())
    assert "periodic" not in dict(on.named_buffers()) and "periodic" not in on.state_dict()
    assert "periodic" not in dict(on.named_parameters())
    # off: the refusal, naming the flag
    with pytest.raises(NotImplementedError, match="periodic=True"):
        off(_cpu_batch(cell=torch.eye(3).unsqueeze(0) * 5))
    # on, without a cell: ValueError before any device work (these are CPU tensors)
    with pytest.raises(ValueError, match="cell"):
        on(_cpu_batch())
    # a plain attribute that may be set after load_state_dict
    off.load_state_dict(on.state_dict())
    off.periodic = True
    with pytest.raises(ValueError, match="cell"):
        off(_cpu_batch())
    # shift and shift_idx are given together
    b = _cpu_batch()
    for kwargs in (dict(shift=torch.zeros(6, 3)), dict(shift_idx=b.edge_shift_idx)):
        with pytest.raises(ValueError, match="together"):
            triplets.xyz_to_dat(b.pos, b.edge_index, 3, True, **kwargs)
        with pytest.raises(ValueError, match="together"):
            triplets.xyz_to_dat_offsets(b.pos, b.edge_index, 3, **kwargs)
    for fn in (triplets.xyz_to_dat, triplets.xyz_to_dat_offsets):
        params = inspect.signature(fn).parameters
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("shift", "shift_idx"))
