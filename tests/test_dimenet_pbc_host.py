"""DimeNet++ on periodic structures, the CPU side: the plain-torch helper tests/dimenet_pbc_ref.py
is pinned (1) to an explicit open-boundary cluster of images enumerated by the unmodified
dimenet_ref.geometry, a path that shares none of the periodic code, and (2) its closed forms of the
vector-form first and second backward to double autograd of its geometry; plus the header, the
ctypes table and the `periodic` flag of the model.  No device work.
"""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import dimenet_pbc_ref as pref
import dimenet_ref as ref
import pbc_ref
from conftest import ROOT

SMALL = dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16)
CELL_1D = np.array([[1.7, 0, 0], [0, 9, 0], [0, 0, 9]], np.float32)
# (name, cell, pbc, atoms, r, layers, E, T, self-image edges, cluster atoms)
STRUCTURES = [
    ("1d-thin", CELL_1D, (True, False, False), 4, 2.0, 2, 36, 290, 8, 52),
    ("thin3d", pbc_ref.THIN, (True, True, True), 3, 2.0, 1, 10, 26, 6, 1617),
]


def _state64(kw, seed=0):
    """A seeded fp64 state dict with random output_blocks.*.lin.weight (PyG's zero
    initialisation would make the output identically zero)."""
    import gmp_amd
    torch.manual_seed(seed)
    sd = {k: v.clone().double() for k, v in gmp_amd.DimeNetPPModel(**kw).state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 100)
    for k in sd:
        if k.startswith("output_blocks.") and k.endswith(".lin.weight"):
            w = sd[k]
            sd[k] = torch.randn(w.shape, generator=gen, dtype=torch.float64) \
                * (2.0 / sum(w.shape)) ** 0.5
    return sd


def _structure(name, cell, pbc, n, r):
    rng = np.random.default_rng(1)
    frac = rng.random((n, 3))
    if name == "1d-thin":  # keep the atoms within reach of each other across the open axes
        frac[:, 1:] = 0.5 + 0.12 * (frac[:, 1:] - 0.5)
    pos = (frac @ cell.astype(np.float64)).astype(np.float32)
    ei, S = pbc_ref.radius_graph_pbc(pos, r, cell, pbc)
    return pos, torch.from_numpy(ei), torch.from_numpy(S).long()


@pytest.mark.parametrize("case", STRUCTURES, ids=[c[0] for c in STRUCTURES])
def test_periodic_helper_equals_explicit_cluster(case):
    """E and F of the periodic helper against the open-boundary cluster: the central cell's atoms
    are graph 0, all replicas within (num_layers + 1) cutoff graph 1; F_periodic[a] is the sum
    over all copies of a of dE_0/dp_copy."""
    name, cell, pbc, n, r, L, n_edges, n_trip, n_self, n_cluster = case
    kw = dict(SMALL, cutoff=r, num_layers=L)
    sd = _state64(kw)
    pos, ei, S = _structure(name, cell, pbc, n, r)
    atoms = torch.tensor([1, 6, 8, 7][:n])
    p = torch.from_numpy(pos).double().requires_grad_(True)
    c = torch.from_numpy(cell).double()
    dist, angle, i, j, kj, ji = pref.geometry(p, c, ei, S)
    assert (ei.shape[1], kj.numel(), int((ei[0] == ei[1]).sum())) == (n_edges, n_trip, n_self)
    coll = pref.collinear(pref.edge_vectors(p.detach(), c, ei, S), kj, ji)
    same_self_image = (kj == ji) & (ei[0] == ei[1])[ji]
    assert torch.equal(coll, same_self_image) and int(coll.sum()) == n_self
    E = ref.model(sd, kw, atoms, dist, angle, i, j, kj, ji, torch.zeros(n, dtype=torch.long), 1)
    (g,) = torch.autograd.grad(E.sum(), p)
    # the explicit cluster
    h = pbc_ref.image_range(pos, cell, pbc, (L + 1) * r)
    imgs = sorted(itertools.product(*[range(-k, k + 1) for k in h]), key=lambda s: s != (0, 0, 0))
    P = torch.cat([torch.from_numpy(pos).double() + torch.tensor(s, dtype=torch.float64) @ c
                   for s in imgs]).requires_grad_(True)
    assert P.shape[0] == n_cluster
    A, orig = atoms.repeat(len(imgs)), torch.arange(n).repeat(len(imgs))
    d = (P.detach()[:, None] - P.detach()[None]).norm(dim=-1)
    src, dst = ((d < r) & ~torch.eye(len(P), dtype=torch.bool)).nonzero(as_tuple=True)
    dist2, angle2, i2, j2, kj2, ji2 = ref.geometry(P, torch.stack([src, dst]))
    in_rest = (torch.arange(len(P)) >= n).long()
    Ec = ref.model(sd, kw, A, dist2, angle2, i2, j2, kj2, ji2, in_rest, 2)
    (gc,) = torch.autograd.grad(Ec[0].sum(), P)
    g_sum = torch.zeros(n, 3, dtype=torch.float64).index_add_(0, orig, gc)
    e_err = float((E - Ec[0]).detach().abs().max())
    f_err = float((g - g_sum).abs().max())
    e_scale, f_scale = max(1.0, float(E.detach().abs().max())), float(g.abs().max())
    print(f"{name}: E err {e_err:.1e} F err {f_err:.1e} of {f_scale:.1e}")
    assert f_scale > 0
    assert e_err <= 1e-10 * e_scale and f_err <= 1e-10 * f_scale


@pytest.mark.parametrize("case", STRUCTURES, ids=[c[0] for c in STRUCTURES])
@pytest.mark.parametrize("cots", ["both", "g_dist", "g_angle"])
def test_closed_forms_equal_double_autograd(case, cots):
    name, cell, pbc, n, r = case[:5]
    pos, ei, S = _structure(name, cell, pbc, n, r)
    c = torch.from_numpy(cell).double()
    vec = pref.edge_vectors(torch.from_numpy(pos).double(), c, ei, S).requires_grad_(True)
    kj, ji = pref.triplets(ei, S)
    E, T = ei.shape[1], kj.numel()
    gen = torch.Generator().manual_seed(7)
    g_dist = torch.randn(E, generator=gen, dtype=torch.float64) if cots != "g_angle" else None
    g_angle = torch.randn(T, generator=gen, dtype=torch.float64) if cots != "g_dist" else None
    a_vec = torch.randn(E, 3, generator=gen, dtype=torch.float64)
    coll = pref.collinear(vec.detach(), kj, ji)
    assert 0 < int(coll.sum()) < T
    if g_angle is not None:  # on an exactly collinear triplet the chain through theta is 0 * inf
        g_angle = (g_angle * ~coll).requires_grad_(True)
    if g_dist is not None:
        g_dist.requires_grad_(True)
    dist, angle = pref.geometry_from_vec(vec, kj, ji)
    obj = sum((g * o).sum() for g, o in ((g_dist, dist), (g_angle, angle)) if g is not None)
    (g_vec,) = torch.autograd.grad(obj, vec, create_graph=True)
    wrt = [t for t in (g_dist, g_angle, vec) if t is not None]
    second = list(torch.autograd.grad((g_vec * a_vec).sum(), wrt))
    det = lambda t: None if t is None else t.detach()  # noqa: E731
    got1 = pref.vec_bwd(vec.detach(), kj, ji, det(g_dist), det(g_angle))
    gg_d, gg_a, h_vec = pref.vec_bwd2(vec.detach(), kj, ji, det(g_dist), det(g_angle), a_vec)

    def close(name, got, want):
        assert bool(torch.isfinite(want).all()), name
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"{name}: {err:.1e} of {scale:.1e}")
        assert scale > 0 and err <= 1e-10 * scale, (name, err, scale)

    close("g_vec", got1, g_vec.detach())
    if g_dist is not None:
        close("gg_dist", gg_d, second.pop(0))
    if g_angle is not None:
        close("gg_angle", gg_a, second.pop(0))
    close("h_vec", h_vec, second.pop(0))


def test_symbols_declared():
    from gmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmp.h")).read()
    for name in ("gmp_triplet_count_pbc", "gmp_triplet_fill_pbc_f32", "gmp_triplet_vec_bwd_f32",
                 "gmp_triplet_vec_bwd2_f32"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 6
    assert re.search(r"#define\s+GMP_ABI_VERSION\s+6\b", header)


def _cpu_batch(**extra):
    from gmp_amd.graph import Batch
    pos = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    ei = torch.tensor([[0, 1, 1, 2, 0, 2], [1, 0, 2, 1, 2, 0]])
    return Batch(torch.ones(3, dtype=torch.long), pos, ei, torch.zeros(3, dtype=torch.long),
                 num_graphs=1, edge_shift_idx=torch.zeros(6, 3, dtype=torch.int32), **extra)


def test_periodic_flag():
    import gmp_amd
    kw = dict(SMALL, num_layers=1)
    on = gmp_amd.DimeNetPPModel(**kw, periodic=True)
    off = gmp_amd.DimeNetPPModel(**kw)
    assert on.periodic is True and off.periodic is False
    sig = inspect.signature(gmp_amd.DimeNetPPModel.__init__)
    assert sig.parameters["periodic"].kind is inspect.Parameter.KEYWORD_ONLY
    # neither a parameter nor a buffer
    assert list(on.state_dict()) == list(off.state_dict())
    assert len(gmp_amd.DimeNetPPModel(periodic=True).state_dict()) == 147
    assert "periodic" not in dict(on.named_buffers()) and "periodic" not in on.state_dict()
    # off: the refusal, naming the flag
    with pytest.raises(NotImplementedError, match="periodic=True"):
        off(_cpu_batch())
    # on, without a cell: ValueError before any device work (these are CPU tensors)
    with pytest.raises(ValueError, match="cell"):
        on(_cpu_batch())
    # a plain attribute that may be set after load_state_dict
    off.load_state_dict(on.state_dict())
    off.periodic = True
    with pytest.raises(ValueError, match="cell"):
        off(_cpu_batch())


def test_spherenet_still_refuses():
    import gmp_amd
    model = gmp_amd.SphereNetModel(hidden_channels=16, int_emb_size=8, out_emb_channels=16,
                                   num_layers=1)
    assert not hasattr(model, "periodic")
    with pytest.raises(NotImplementedError):
        model(_cpu_batch(cell=torch.eye(3).unsqueeze(0) * 5))
