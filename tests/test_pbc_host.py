"""Periodic boundary conditions, host side (no GPU): the brute-force reference of the contract
(tests/pbc_ref.py) against known coordination numbers and its own symmetries, the grid plan of
the device builder against fp64 heights, the public surface, and the yardstick of the stress
tests: the fp64 periodic SchNet oracle's strain derivative against central differences."""
import numpy as np
import pytest
import torch

import pbc_ref
from oracle import radius as oradius


# ------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("cell,pbc,r,edges", pbc_ref.KNOWN)
def test_reference_known_answers(cell, pbc, r, edges):
    """Coordination shells: simple cubic within 2.5 a (6 + 12 + 8 + 6 + 24 + 24 = 80), fcc first
    shell (12) and first two (18), the square lattice of a slab within 1.5 a (4 + 4)."""
    ei, S = pbc_ref.radius_graph_pbc(np.zeros((1, 3), np.float32), r, cell, pbc)
    assert ei.shape[1] == edges and (ei == 0).all()
    assert len({tuple(s) for s in S}) == edges and not (S == 0).all(1).any()
    assert all(S[:, k].max() == 0 and S[:, k].min() == 0 for k in range(3) if not pbc[k])


def _structure(seed=0, n=40, cell=pbc_ref.TRICLINIC):
    return pbc_ref.random_in_cell(n, cell, seed)


def test_reference_is_symmetric_and_sorted():
    pos = _structure()
    ei, S = pbc_ref.radius_graph_pbc(pos, 2.0, pbc_ref.TRICLINIC)
    fwd = {(int(j), int(i), *map(int, s)) for j, i, s in zip(ei[0], ei[1], S)}
    assert len(fwd) == ei.shape[1] > 100
    assert fwd == {(i, j, -a, -b, -c) for j, i, a, b, c in fwd}
    key = np.stack([ei[1], ei[0], S[:, 0], S[:, 1], S[:, 2]], 1)
    assert (np.lexsort(key.T[::-1]) == np.arange(len(key))).all()


@pytest.mark.parametrize("cell,r", [(pbc_ref.TRICLINIC, 2.0), (pbc_ref.THIN, 2.0)])
def test_reference_one_more_shell_changes_nothing(cell, r):
    pos = _structure(1, 12, cell)
    a = pbc_ref.radius_graph_pbc(pos, r, cell)
    b = pbc_ref.radius_graph_pbc(pos, r, cell, extra=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_reference_vacuum_cell_is_the_open_graph():
    rng = np.random.default_rng(3)
    pos = (rng.random((60, 3)) * 6 + 40).astype(np.float32)
    batch = np.repeat([0, 1], 30)
    cell = np.stack([np.eye(3, dtype=np.float32) * 100] * 2)
    ei, S = pbc_ref.radius_graph_pbc(pos, 2.0, cell, batch=batch)
    assert np.array_equal(ei, oradius.radius_graph(pos, 2.0, batch, max_num_neighbors=0))
    assert ei.shape[1] > 50 and (S == 0).all()


def _small_oracle(cutoff=2.0):
    torch.manual_seed(5)
    m = pbc_ref.PeriodicSchNet(hidden_channels=16, num_filters=16, num_layers=2,
                               num_gaussians=10, cutoff=cutoff, out_dim=1).double()
    with torch.no_grad():
        m.embedding.weight.normal_()
    return m


def _oracle_energy(model, atoms, pos, cell, r):
    from gmp_amd.graph import Batch
    ei, S = pbc_ref.radius_graph_pbc(pos, r, cell)
    shift = torch.from_numpy(S).double() @ torch.from_numpy(np.asarray(cell)).double()
    b = Batch(atoms, torch.from_numpy(pos).double(), torch.from_numpy(ei), num_graphs=1,
              edge_shift=shift)
    return ei.shape[1], model(b).item()


def test_reference_displaced_atoms_keep_edges_and_energy():
    """Moving atoms by +-2 lattice vectors changes no physics: same edge count, same fp64 energy
    (pos in multiples of 1/64 and a dyadic cell, so the moves are exact in fp32)."""
    cell = np.array([[4, 0, 0], [1, 3.5, 0], [-0.5, 0.75, 5]], np.float32)
    rng = np.random.default_rng(7)
    pos = (np.round(rng.random((14, 3)) @ cell * 64) / 64).astype(np.float32)
    move = rng.integers(-2, 3, (14, 3)).astype(np.float32)
    moved = pos + move @ cell
    atoms = torch.from_numpy(rng.integers(1, 5, 14))
    model = _small_oracle()
    n0, e0 = _oracle_energy(model, atoms, pos, cell, 2.0)
    n1, e1 = _oracle_energy(model, atoms, moved, cell, 2.0)
    assert n0 == n1 > 50
    assert abs(e0 - e1) <= 1e-12 * max(1.0, abs(e0))


# ------------------------------------------------------------------------------ the grid plan
PLAN_CELLS = {
    "orthorhombic": (np.diag([9.0, 12.0, 20.0]), (True, True, True), 2.5),
    "triclinic": (pbc_ref.TRICLINIC.astype(np.float64), (True, True, True), 2.0),
    "thin": (pbc_ref.THIN.astype(np.float64), (True, True, True), 2.0),
    "mixed": (np.array([[7.0, 0, 0], [2.0, 8.0, 0], [0.5, 0.5, 30.0]]), (True, True, False), 2.0),
}


@pytest.mark.parametrize("name", list(PLAN_CELLS))
def test_grid_plan(name):
    """heights against 1 / |column k of inv(cell)| in fp64; every bin at least r (1 + eps) wide;
    the reach covers r (1 + eps) and is minimal; the table stays near 2 bins per node."""
    from gmp_amd.graph import pbc_grid_plan, PBC_EPS
    cell, pbc, r = PLAN_CELLS[name]
    n = 50
    lo, hi = np.array([[0.0, 0.0, 0.2]]), np.array([[1.0, 1.0, 0.8]])
    p = pbc_grid_plan(cell[None], pbc, r, counts=[n], frac_lo=lo, frac_hi=hi,
                      pos_absmax=np.abs(cell).sum(0)[None])
    h = 1.0 / np.linalg.norm(np.linalg.inv(cell), axis=0)
    assert np.allclose(p["heights"][0], h, rtol=1e-12)
    assert np.isclose(p["volume"][0], abs(np.linalg.det(cell)), rtol=1e-12)
    rr = r * (1 + PBC_EPS)
    nb, m = p["nb"][0], p["m"][0]
    assert (nb >= 1).all() and nb.prod() <= 2 * n + 8 and p["base"].tolist() == [0, nb.prod()]
    for k in range(3):
        if pbc[k]:
            w = h[k] / nb[k]
            assert m[k] * w >= rr and (m[k] - 1) * w < rr
            assert nb[k] == 1 or w >= rr
            assert p["org"][0, k] == 0 and p["scale"][0, k] == nb[k]
        else:
            w = (hi[0, k] - lo[0, k]) * h[k] / nb[k]
            assert nb[k] == 1 or w >= rr
            assert m[k] == (1 if nb[k] > 1 else 0) and p["org"][0, k] == lo[0, k]
    if name == "thin":
        assert m[0] == 2 and nb[0] == 1  # h_0 = 1.59 < r
    if name == "orthorhombic":
        assert nb.tolist() == [3, 4, 7] and m.tolist() == [1, 1, 1]


def test_grid_plan_refusals():
    from gmp_amd.graph import pbc_grid_plan
    eye = np.eye(3)[None]
    with pytest.raises(ValueError, match="cell"):
        pbc_grid_plan(np.eye(3), (1, 1, 1), 1.0)
    with pytest.raises(ValueError, match="singular"):
        pbc_grid_plan(np.array([[[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]]), (1, 1, 1), 1.0)
    with pytest.raises(ValueError, match="r must"):
        pbc_grid_plan(eye, (1, 1, 1), 0.0)
    with pytest.raises(ValueError, match="images"):      # reach 200 > 127
        pbc_grid_plan(eye * 0.01, (1, 1, 1), 2.0)
    with pytest.raises(ValueError, match="cells apart"):  # wrap 200 > 127
        pbc_grid_plan(eye, (1, 1, 1), 0.5, frac_lo=np.zeros((1, 3)), frac_hi=np.full((1, 3), 200.))
    with pytest.raises(ValueError, match="margin"):      # |frac| * nb = 100 * 20 > 700
        pbc_grid_plan(eye * 10, (1, 1, 1), 0.5, counts=[10 ** 6], frac_lo=np.zeros((1, 3)),
                      frac_hi=np.full((1, 3), 100.), pos_absmax=np.full((1, 3), 1000.))
    pbc_grid_plan(eye * 0.02, (1, 1, 1), 2.0)  # reach 101: still fine


# ------------------------------------------------------------------------------ public surface
def test_public_names_and_argument_errors():
    import gmp_amd
    from gmp_amd import ops
    for name in ("radius_graph_pbc_gpu", "pbc_grid_plan", "energy_and_forces"):
        assert hasattr(gmp_amd, name), name
    assert hasattr(ops, "edge_shift_vectors")
    pos, eye = torch.zeros(4, 3), torch.eye(3)
    f = gmp_amd.radius_graph_pbc_gpu
    with pytest.raises(ValueError, match="cell"):
        f(pos, 1.0, torch.eye(4))
    with pytest.raises(ValueError, match="one cell per graph"):
        f(pos, 1.0, eye, batch=torch.tensor([0, 0, 1, 1]), num_graphs=2)
    with pytest.raises(ValueError, match="singular"):
        f(pos, 1.0, torch.zeros(3, 3))
    with pytest.raises(ValueError, match="r must"):
        f(pos, -1.0, eye)
    with pytest.raises(ValueError, match="images"):
        f(pos, 2.0, eye * 0.01)


def _periodic_graph(seed, n=6):
    from gmp_amd.graph import Batch
    cell = torch.from_numpy(pbc_ref.THIN)
    pos = pbc_ref.random_in_cell(n, pbc_ref.THIN, seed)
    ei, S = pbc_ref.radius_graph_pbc(pos, 2.0, pbc_ref.THIN)
    return Batch(torch.ones(n, dtype=torch.long), torch.from_numpy(pos), torch.from_numpy(ei),
                 num_graphs=1, cell=cell, pbc=(True, True, True),
                 edge_shift_idx=torch.from_numpy(S))


def test_collate_carries_the_periodic_fields():
    from gmp_amd.graph import Batch, collate
    a, b = _periodic_graph(1), _periodic_graph(2, 5)
    c = collate([a, b])
    assert tuple(c.cell.shape) == (2, 3, 3) and c.pbc == (True, True, True)
    assert c.edge_shift_idx.dtype == torch.int32
    assert torch.equal(c.edge_shift_idx, torch.cat([a.edge_shift_idx, b.edge_shift_idx]))
    assert c.edge_index.shape[1] == c.edge_shift_idx.shape[0]
    assert c.to("cpu").cell is not None
    open_graph = Batch(a.atoms, a.pos, a.edge_index, num_graphs=1)
    mixed = collate([a, open_graph])  # not every graph has them: none are carried
    assert mixed.cell is None and mixed.edge_shift_idx is None
    b.pbc = (True, True, False)
    with pytest.raises(ValueError, match="pbc"):
        collate([a, b])


@pytest.mark.parametrize("name", ["EGNNModel", "GVPGNNModel"])
def test_models_without_images_refuse_them(name):
    """Before any device call: the batch is on the CPU, where every kernel would raise GmpError."""
    import gmp_amd
    model = getattr(gmp_amd, name)(num_layers=1, emb_dim=8) if name == "EGNNModel" else \
        getattr(gmp_amd, name)(num_layers=1)
    with pytest.raises(NotImplementedError, match="periodic"):
        model(_periodic_graph(3))


# ------------------------------------------------------------------------------ the yardstick
def test_oracle_stress_matches_central_differences():
    """sigma = (1 / V) dE / d eps of the fp64 periodic SchNet oracle under the symmetric strain,
    by autograd, against central differences of E in each of the nine entries of eps: 12 atoms
    in a triclinic cell thinner than r, so self-image edges take part.  1e-6 of scale
    (measured ~1e-9)."""
    from gmp_amd.graph import Batch
    cell_np, r, n = pbc_ref.THIN, 2.0, 12
    pos_np = pbc_ref.random_in_cell(n, cell_np, 11)
    ei_np, S_np = pbc_ref.radius_graph_pbc(pos_np, r, cell_np)
    assert np.abs(S_np).max() >= 1 and (ei_np[0] == ei_np[1]).any()
    model = _small_oracle(r)
    atoms = torch.from_numpy(np.random.default_rng(2).integers(1, 5, n))
    pos = torch.from_numpy(pos_np).double().requires_grad_(True)
    cell = torch.from_numpy(cell_np).double().view(1, 3, 3)
    ei, S = torch.from_numpy(ei_np), torch.from_numpy(S_np)
    batch = torch.zeros(n, dtype=torch.long)
    E, F, sigma = pbc_ref.oracle_energy_forces_stress(model, atoms, pos, cell, ei, S, batch, 1)

    def energy(eps):
        sym = 0.5 * (eps + eps.t())
        p, c = pos.detach() + pos.detach() @ sym, cell[0] + cell[0] @ sym
        b = Batch(atoms, p, ei, batch, num_graphs=1, edge_shift=S.double() @ c)
        return model(b).item()

    h, fd = 1e-5, torch.zeros(3, 3, dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            d = torch.zeros(3, 3, dtype=torch.float64)
            d[a, b] = h
            fd[a, b] = (energy(d) - energy(-d)) / (2 * h)
    fd = fd / abs(np.linalg.det(cell_np.astype(np.float64)))
    scale = fd.abs().max().item()
    err = (sigma[0] - fd).abs().max().item()
    print(f"stress: max|d| = {err:.3e}, scale {scale:.3e}")
    assert scale > 1e-4 and err <= 1e-6 * scale
    assert torch.equal(sigma[0], sigma[0].t()) or (sigma[0] - sigma[0].t()).abs().max() < 1e-14
    assert F.sum(0).abs().max().item() <= 1e-10 * max(F.abs().max().item(), 1e-30) + 1e-14
