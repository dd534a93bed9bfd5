"""Periodic boundary conditions on the GPU: the device builder (gmp_radius_pbc_*) bit for bit
against the brute-force reference of the contract (tests/pbc_ref.py), the featurisation kernels
with a per-edge shift against fp64 autograd, SchNet / MACE / TFN energies, forces and stresses
against the fp64 periodic oracles, and symmetry properties at 2k atoms.  Tolerances are the
project's: 1e-5 on outputs, 1e-4 of scale on gradient quantities."""
import copy
import itertools
import math

import numpy as np
import pytest
import torch

import pbc_ref
from oracle import mace as om
from oracle import o3 as oo3
from oracle import schnet as osch
from oracle.radial import RadialEmbeddingBlock as ORadial

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = (True, True, True)


def _scaled(a, b, rtol, name):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    print(f"{name}: max|d|={err:.3e} scale={scale:.3e} ({err / scale:.2e} of scale)")
    assert err <= rtol * scale + 1e-6, f"{name}: max|d|={err:.3e} scale={scale:.3e}"


def _build(pos, r, cell, pbc=ALL, batch=None, num_graphs=None):
    import gmp_amd
    ei, S = gmp_amd.radius_graph_pbc_gpu(
        torch.as_tensor(pos).to(DEV), r, torch.as_tensor(cell), pbc,
        None if batch is None else torch.as_tensor(batch).to(DEV), num_graphs)
    assert ei.dtype == torch.int64 and S.dtype == torch.int32
    assert ei.shape == (2, S.shape[0]) and S.shape[1:] == (3,)
    return ei.cpu(), S.cpu()


def _check(pos, r, cell, pbc=ALL, batch=None, num_graphs=None):
    ei, S = _build(pos, r, cell, pbc, batch, num_graphs)
    rei, rS = pbc_ref.radius_graph_pbc(pos, r, cell, pbc, batch)
    print(f"E = {rei.shape[1]}")
    assert ei.shape[1] == rei.shape[1]
    assert torch.equal(ei, torch.from_numpy(rei)) and torch.equal(S, torch.from_numpy(rS))
    return rei, rS


# ------------------------------------------------------------------------------------ builder
@pytest.mark.parametrize("cell,pbc,r,edges", pbc_ref.KNOWN)
def test_builder_known_answers(cell, pbc, r, edges):
    rei, _ = _check(np.zeros((1, 3), np.float32), r, cell, pbc)
    assert rei.shape[1] == edges


def test_builder_triclinic_200():
    _check(pbc_ref.random_in_cell(200, pbc_ref.TRICLINIC, 0), 2.0, pbc_ref.TRICLINIC)


def test_builder_slab():
    _, S = _check(pbc_ref.random_in_cell(100, pbc_ref.TRICLINIC, 1), 2.0, pbc_ref.TRICLINIC,
                  (True, True, False))
    assert (S[:, 2] == 0).all() and (S[:, :2] != 0).any()


VERY_THIN = np.array([[0.9, 0, 0], [0.3, 5.5, 0], [-0.2, 1.1, 6.0]], np.float32)  # r / h_0 > 2


def test_builder_three_graphs():
    """One batch: a cell thinner than r / 2 (reach 3 along its axis, |S| >= 2), a many-bin cell
    and a graph of a single atom (edges only to its own images)."""
    pos = np.concatenate([pbc_ref.random_in_cell(10, VERY_THIN, 2),
                          pbc_ref.random_in_cell(120, np.eye(3) * 12, 3),
                          np.array([[.1, .2, .3]], np.float32)])
    batch = np.array([0] * 10 + [1] * 120 + [2])
    cells = np.stack([VERY_THIN, np.eye(3, dtype=np.float32) * 12, pbc_ref.FCC])
    rei, S = _check(pos, 2.0, cells, batch=batch, num_graphs=3)
    assert np.abs(S[:, 0]).max() >= 2 and (rei[1] == 130).sum() > 12
    ei2, S2 = _build(pos, 2.0, cells, batch=batch)  # num_graphs read from batch
    assert torch.equal(ei2, torch.from_numpy(rei)) and torch.equal(S2, torch.from_numpy(S))


def _dyadic(n, cell, seed):
    rng = np.random.default_rng(seed)
    return (np.round(rng.random((n, 3)) @ cell * 64) / 64).astype(np.float32)


DYADIC = np.array([[4, 0, 0], [1, 3.5, 0], [-.5, .75, 5]], np.float32)


def test_builder_displaced_atoms():
    """Atoms moved by +-2 lattice vectors (exactly, dyadic numbers): the same edges between
    other images, S_moved = S + move_i - move_j."""
    pos = _dyadic(40, DYADIC, 5)
    move = np.random.default_rng(6).integers(-2, 3, (40, 3))
    rei0, S0 = _check(pos, 2.0, DYADIC)
    rei1, S1 = _check(pos + move.astype(np.float32) @ DYADIC, 2.0, DYADIC)
    assert np.array_equal(rei0, rei1)
    key = lambda ei, S: sorted(zip(ei[1], ei[0], *S.T))
    assert key(rei1, S1) == key(rei0, S0 + move[rei0[1]] - move[rei0[0]])


@pytest.mark.parametrize("pbc", [ALL, (True, False, True)])
def test_builder_faces_corners_bin_boundaries_duplicates(pbc):
    g = np.array(list(itertools.product([0, .5, 1, 1.5, 2, 3, 4], repeat=3)), np.float32)[::3]
    g = np.concatenate([g, g[:5]])  # coincident distinct atoms are neighbours
    rei, S = _check(g, 1.0, np.eye(3, dtype=np.float32) * 4, pbc)
    dup = (rei[0] == len(g) - 5) & (rei[1] == 0) & (S == 0).all(1)
    assert dup.sum() == 1


def test_builder_empty():
    ei, S = _build(np.zeros((0, 3), np.float32), 1.0, pbc_ref.CUBIC)
    assert ei.shape == (2, 0) and S.shape == (0, 3)
    ei, S = _build(np.array([[0, 0, 0], [5, 5, 5]], np.float32), 1.0, np.eye(3) * 10)
    assert ei.shape == (2, 0) and S.shape == (0, 3)  # nodes, no edges


@pytest.mark.parametrize("n,box,r", [(60, 4.0, 1.55), (60, 4.0, 3.0), (32, 2.0, 3.9),
                                     (32, 2.0, 3.95), (32, 2.0, 4.2)])
def test_builder_degree_thresholds(n, box, r):
    """Degrees on each side of what the fill kernel distinguishes: below and above one wave's 64
    lanes (~15 and ~106 per atom), and around the LDS sort capacity (~994, ~1033 and ~1241 per
    atom in a 2^3 cell: in LDS, mixed, in global memory)."""
    from gmp_amd import _lib
    cap = _lib.load().gmp_radius_pbc_sort_capacity()
    assert cap == 1024
    rei, _ = _check(pbc_ref.random_in_cell(n, np.eye(3) * box, n), r, np.eye(3) * box)
    deg = np.bincount(rei[1], minlength=n)
    print(f"degrees {deg.min()}..{deg.max()}")
    want = {1.55: deg.max() < 64, 3.0: 64 < deg.min() and deg.max() < cap,
            3.9: 900 < deg.min() and deg.max() <= cap, 3.95: deg.min() <= cap < deg.max(),
            4.2: deg.min() > cap}[r]
    assert want, (deg.min(), deg.max())


def test_builder_vacuum_cell_is_the_open_builder():
    import gmp_amd
    rng = np.random.default_rng(3)
    pos = torch.from_numpy((rng.random((3000, 3)) * 20 + 40).astype(np.float32)).to(DEV)
    batch = torch.from_numpy(np.repeat([0, 1, 2], 1000)).to(DEV)
    cell = torch.eye(3).repeat(3, 1, 1) * 100
    ei, S = gmp_amd.radius_graph_pbc_gpu(pos, 2.0, cell, batch=batch, num_graphs=3)
    ref = gmp_amd.radius_graph_gpu(pos, 2.0, batch, max_num_neighbors=None, num_graphs=3)
    assert ei.shape[1] > 3000 and torch.equal(ei, ref) and not S.any()


def test_builder_dyadic_supercell():
    """pos in multiples of 1/64 and cell in multiples of 1/4: all arithmetic is exact, so the
    2 x 1 x 1 supercell's list is exactly the image of the cell's list: the edge (j -> i, S) and
    the copy c_i of i give (j + n c_j -> i + n c_i, ((S0 + c_i - c_j) / 2, S1, S2)) with
    c_j = (S0 + c_i) mod 2."""
    n = 30
    pos = _dyadic(n, DYADIC, 8)
    ei, S = _build(pos, 2.0, DYADIC)
    sup_cell = DYADIC * np.array([[2], [1], [1]], np.float32)
    ei2, S2 = _build(np.concatenate([pos, pos + DYADIC[0]]), 2.0, sup_cell)
    want = set()
    for (j, i), s in zip(ei.t().tolist(), S.tolist()):
        for ci in (0, 1):
            cj = (s[0] + ci) % 2
            want.add((j + n * cj, i + n * ci, (s[0] + ci - cj) // 2, s[1], s[2]))
    got = {(j, i, *s) for (j, i), s in zip(ei2.t().tolist(), S2.tolist())}
    assert len(got) == ei2.shape[1] == 2 * ei.shape[1] and got == want


def test_builder_20k_atoms():
    """20k atoms, ~400k edges, cubic.  Reference: the 27 images, cKDTree candidates within
    r (1 + 1e-4), then the contract's exact fp32 test."""
    from scipy.spatial import cKDTree
    n, L, r = 20000, 40.0, 2.5
    cell = np.eye(3, dtype=np.float32) * L
    pos = pbc_ref.random_in_cell(n, cell, 12)
    ei, S = _build(pos, r, cell)
    shifts = np.array(list(itertools.product((-1, 0, 1), repeat=3)), np.int32)
    images = (pos[None].astype(np.float64) + shifts[:, None] @ cell.astype(np.float64))
    tree = cKDTree(images.reshape(-1, 3))
    hits = tree.query_ball_point(pos.astype(np.float64), r * (1 + 1e-4))
    i = np.repeat(np.arange(n), [len(h) for h in hits])
    flat = np.concatenate(hits)
    j, Sj = flat % n, shifts[flat // n]
    d = (pos[i] - pos[j]) - pbc_ref.shift_vectors(Sj, cell)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = (d2 < np.float32(r) * np.float32(r)) & ~((i == j) & (Sj == 0).all(1))
    i, j, Sj = i[keep], j[keep], Sj[keep]
    order = np.lexsort((Sj[:, 2], Sj[:, 1], Sj[:, 0], j, i))
    print(f"E = {len(order)}")
    assert 350_000 < len(order) < 450_000
    assert torch.equal(ei, torch.from_numpy(np.stack([j[order], i[order]])))
    assert torch.equal(S, torch.from_numpy(Sj[order]))


# ------------------------------------------------------------------------------------ kernels
def _edges(E, cutoff, seed):
    gen = torch.Generator().manual_seed(seed)
    n = max(E // 20, 4)
    pos = torch.rand(n, 3, generator=gen) * 1.5 * cutoff
    ei = torch.randint(0, n, (2, E), generator=gen)
    shift = (torch.rand(E, 3, generator=gen) - 0.5) * cutoff
    return pos, ei, shift, gen


def _schnet_ref(v, off, coeff, cutoff):
    d = v.norm(dim=-1)
    t = d[:, None] - off[None, :]
    return d, torch.exp(coeff * t * t), 0.5 * (torch.cos(d * math.pi / cutoff) + 1.0)


@pytest.mark.parametrize("E,G,cutoff", [(20000, 50, 10.0), (333, 7, 4.0), (0, 50, 10.0)])
def test_schnet_featurize_with_shift_vs_fp64(E, G, cutoff):
    """Forward, backward and second backward of the SchNet featurisation with a shift, against
    fp64 autograd of the formula on v = pos[a] - pos[b] + shift (built as
    tests/test_gpu_forces.py::test_schnet_featurize_bwd2_vs_fp64 builds it; 1e-4 of scale)."""
    from gmp_amd import _lib
    tops = _lib.torch_ops()
    pos, ei, shift, gen = _edges(E, cutoff, E + G)
    gs = osch.GaussianSmearing(0.0, cutoff, G)
    g_d, g_cut = torch.randn(E, generator=gen), torch.randn(E, generator=gen)
    g_rbf, a = torch.randn(E, G, generator=gen), torch.randn(E, 3, generator=gen)
    dv = lambda t: t.to(DEV)
    args = (dv(pos), dv(ei), dv(gs.offset), gs.coeff, cutoff)
    fwd = tops.schnet_featurize(*args, dv(shift))
    gv = tops.schnet_featurize_bwd(*args, dv(g_d), dv(g_rbf), dv(g_cut), dv(shift))
    out2 = tops.schnet_featurize_bwd2(*args, dv(g_d), dv(g_rbf), dv(g_cut), dv(a), True, True,
                                      True, True, dv(shift))
    assert [tuple(t.shape) for t in fwd] == [(E,), (E, G), (E,)] and gv.shape == (E, 3)
    assert [tuple(t.shape) for t in out2] == [(E,), (E, G), (E,), (E, 3)]
    if E == 0:
        return
    f64 = lambda t: t.double().requires_grad_(True)
    v = f64(pos.double()[ei[0]] - pos.double()[ei[1]] + shift.double())
    rd, rr, rc = f64(g_d), f64(g_rbf), f64(g_cut)
    ref = _schnet_ref(v, gs.offset.double(), gs.coeff, cutoff)
    for got, want, name in zip(fwd, ref, ("dist", "rbf", "cut")):
        _scaled(got, want, 1e-4, name)
    (gv64,) = torch.autograd.grad((ref[0] * rd).sum() + (ref[1] * rr).sum() + (ref[2] * rc).sum(),
                                  v, create_graph=True)
    _scaled(gv, gv64, 1e-4, "g_vec")
    refs = torch.autograd.grad((gv64 * a.double()).sum(), [rd, rr, rc, v])
    for got, want, name in zip(out2, refs, ("gg_d", "gg_rbf", "gg_cut", "h_vec")):
        _scaled(got, want, 1e-4, name)


def test_schnet_shift_cotangent_is_g_vec_and_zero_shift_is_bitwise():
    """Through the autograd Functions: d/d shift is the kernel's g_vec itself (h_vec in the
    second backward), and shift = zeros gives bitwise what shift = None gives (no zero-length
    edge here: -0.0 + 0.0 is the only place the two could differ)."""
    from gmp_amd import _lib, ops
    tops = _lib.torch_ops()
    E, G, cutoff = 5000, 50, 10.0
    pos, ei, shift, gen = _edges(E, cutoff, 77)
    ei[1] = (ei[0] + 1 + ei[1] % (pos.shape[0] - 1)) % pos.shape[0]  # no self-loops
    gs = osch.GaussianSmearing(0.0, cutoff, G)
    cots = [torch.randn(E, generator=gen).to(DEV), torch.randn(E, G, generator=gen).to(DEV),
            torch.randn(E, generator=gen).to(DEV)]
    a = torch.randn(E, 3, generator=gen).to(DEV)
    pos_d, ei_d, off = pos.to(DEV), ei.to(DEV), gs.offset.to(DEV)
    for fn in (ops.SchNetFeaturizeFn, ops.SchNetFeaturize2Fn):
        sh = shift.to(DEV).requires_grad_(True)
        p = pos_d.clone().requires_grad_(True)
        outs = fn.apply(p, ei_d, off, gs.coeff, cutoff, sh)
        second = fn is ops.SchNetFeaturize2Fn
        g_p, g_sh = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), (p, sh),
                                        create_graph=second)
        g_vec = tops.schnet_featurize_bwd(pos_d, ei_d, off, gs.coeff, cutoff, *cots, sh.detach())
        assert torch.equal(g_sh.detach(), g_vec)
        assert torch.equal(g_p.detach(), ops.edge_vec_to_pos_grad(g_vec, ei_d, pos.shape[0]))
        if second:
            (h_sh,) = torch.autograd.grad((g_sh * a).sum(), sh)
            h_vec = tops.schnet_featurize_bwd2(pos_d, ei_d, off, gs.coeff, cutoff, *cots, a,
                                               False, False, False, True, sh.detach())[3]
            assert torch.equal(h_sh, h_vec)
    zero = torch.zeros(E, 3, device=DEV)
    base = (pos_d, ei_d, off, gs.coeff, cutoff)
    for x, y in zip(tops.schnet_featurize(*base), tops.schnet_featurize(*base, zero)):
        assert torch.equal(x, y)
    assert torch.equal(tops.schnet_featurize_bwd(*base, *cots),
                       tops.schnet_featurize_bwd(*base, *cots, zero))
    for x, y in zip(tops.schnet_featurize_bwd2(*base, *cots, a),
                    tops.schnet_featurize_bwd2(*base, *cots, a, True, True, True, True, zero)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("lmax", [2, 3, 1, 4, 5])
def test_k1_featurize_with_shift_vs_oracle(lmax):
    """K1 (TFN / MACE) with a shift, as tests/test_gpu_equivariant.py::test_featurize_vs_oracle
    checks the open path, at its 1e-5; the cotangent of shift is the kernel's g_vec; zeros are
    bitwise None."""
    from gmp_amd import _lib, equivariant as eq
    from gmp_amd.graph import radius_graph
    g = radius_graph(num_nodes=500, target_edges=8000, r=2.0, seed=3, tol=0.2, shuffle=True)
    gen = torch.Generator().manual_seed(lmax)
    # a shift that keeps |vec| inside the radial cutoff's interesting range
    shift = (torch.rand(g.num_edges, 3, generator=gen) - 0.5) * 0.6
    rad_p, rad_o = eq.RadialEmbeddingBlock(2.0, 8, 5), ORadial(2.0, 8, 5)
    pos_d = g.pos.to(DEV).requires_grad_(True)
    sh_d = shift.to(DEV).requires_grad_(True)
    ei_d = g.edge_index.to(DEV)
    graph = eq.tp_graph(ei_d, g.num_nodes)
    sh, rad = eq.EdgeFeaturizeFn.apply(pos_d, ei_d, rad_p._host, graph, lmax, sh_d)
    pos_o, shift_o = g.pos.clone().requires_grad_(True), shift.clone().requires_grad_(True)
    vec = pos_o[g.edge_index[0]] - pos_o[g.edge_index[1]] + shift_o
    sh_o = oo3.spherical_harmonics(vec, lmax)
    rad_o_v = rad_o(torch.linalg.norm(vec, dim=-1, keepdim=True))
    torch.testing.assert_close(sh.cpu(), sh_o.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(rad.cpu(), rad_o_v.detach(), atol=1e-5, rtol=1e-5)
    torch.manual_seed(lmax)
    gs, gr = torch.randn_like(sh_o), torch.randn_like(rad_o_v)
    ((sh * gs.to(DEV)).sum() + (rad * gr.to(DEV)).sum()).backward()
    ((sh_o * gs).sum() + (rad_o_v * gr).sum()).backward()
    _scaled(pos_d.grad, pos_o.grad, 1e-5, "dpos")
    _scaled(sh_d.grad, shift_o.grad, 1e-5, "dshift")
    w, pref, r_max, p = rad_p._host
    consts = ([float(v) for v in w], pref, r_max, p)
    tops = _lib.torch_ops()
    g_vec = tops.edge_featurize_bwd(pos_d.detach(), ei_d, *consts, gs.to(DEV), gr.to(DEV), lmax,
                                    sh_d.detach())
    assert torch.equal(sh_d.grad, g_vec)
    zero = torch.zeros_like(shift).to(DEV)
    for x, y in zip(tops.edge_featurize(pos_d.detach(), ei_d, *consts, lmax),
                    tops.edge_featurize(pos_d.detach(), ei_d, *consts, lmax, zero)):
        assert torch.equal(x, y)
    assert torch.equal(
        tops.edge_featurize_bwd(pos_d.detach(), ei_d, *consts, gs.to(DEV), gr.to(DEV), lmax),
        tops.edge_featurize_bwd(pos_d.detach(), ei_d, *consts, gs.to(DEV), gr.to(DEV), lmax, zero))


def test_edge_shift_vectors():
    """t bitwise the contract's fp32 formula; d cell = sum_e S_e (x) g_e per graph against fp64;
    the transpose pair is twice differentiable."""
    from gmp_amd import ops
    gen = torch.Generator().manual_seed(9)
    E, B = 7001, 3
    S = torch.randint(-127, 128, (E, 3), generator=gen, dtype=torch.int32)
    graph = torch.randint(0, B, (E,), generator=gen)
    cell = torch.randn(B, 3, 3, generator=gen) * 3
    cell_d = cell.to(DEV).requires_grad_(True)
    t = ops.edge_shift_vectors(S.to(DEV), cell_d, graph.to(DEV))
    want = pbc_ref.shift_vectors(S.numpy(), cell.numpy()[graph.numpy()])
    assert torch.equal(t.detach().cpu(), torch.from_numpy(want))
    g = torch.randn(E, 3, generator=gen)
    (dc,) = torch.autograd.grad((t * g.to(DEV)).sum(), cell_d, create_graph=True)
    ref = torch.zeros(B, 3, 3, dtype=torch.float64).index_add(
        0, graph, S.double()[:, :, None] * g.double()[:, None, :])
    _scaled(dc, ref, 1e-4, "dcell")
    g2 = g.to(DEV).requires_grad_(True)
    (dc2,) = torch.autograd.grad((ops.edge_shift_vectors(S.to(DEV), cell_d, graph.to(DEV)) * g2)
                                 .sum(), cell_d, create_graph=True)
    a = torch.randn(B, 3, 3, generator=gen)
    (back,) = torch.autograd.grad((dc2 * a.to(DEV)).sum(), g2)  # = S . a[graph]
    _scaled(back, torch.einsum("ek,ekc->ec", S.double(), a.double()[graph]), 1e-5, "transpose")
    one = ops.edge_shift_vectors(S[:5].to(DEV), cell[:1].to(DEV))  # single graph: no edge_graph
    assert torch.equal(one.cpu(), torch.from_numpy(pbc_ref.shift_vectors(S[:5].numpy(),
                                                                       cell[0].numpy())))


# ------------------------------------------------------------------------------------ models
_C1 = dict(hidden_channels=64, num_filters=128, num_layers=4, num_gaussians=50, cutoff=10,
           out_dim=1)
_REF = {}


def _two_graphs(r=3.0, n=60):
    """Two triclinic graphs of n atoms, the second in a cell thinner than the cutoff."""
    if "graphs" not in _REF:
        from gmp_amd.graph import Batch, collate
        gs = []
        for k, cell in enumerate((pbc_ref.TRICLINIC, pbc_ref.THIN)):
            pos = pbc_ref.random_in_cell(n, cell, 20 + k)
            ei, S = pbc_ref.radius_graph_pbc(pos, r, cell)
            atoms = torch.randint(1, 5, (n,), generator=torch.Generator().manual_seed(k))
            gs.append(Batch(atoms, torch.from_numpy(pos), torch.from_numpy(ei), num_graphs=1,
                            cell=torch.from_numpy(cell), pbc=ALL,
                            edge_shift_idx=torch.from_numpy(S)))
        _REF["graphs"] = collate(gs)
        assert (gs[1].edge_index[0] == gs[1].edge_index[1]).any()  # self-image edges
    return _REF["graphs"]


def _targets(b):
    gen = torch.Generator().manual_seed(17)
    return (torch.randn(b.num_graphs, 1, generator=gen),
            torch.randn(b.pos.shape[0], 3, generator=gen),
            torch.randn(b.num_graphs, 3, 3, generator=gen) * 0.01)


def _loss(E, F, sigma, tg, loss):
    y, Fs, ss = tg
    lf = ((F - Fs) ** 2).sum() + ((sigma - ss) ** 2).sum()
    return lf if loss == "force" else (E - y).abs().sum() + lf


def _grad(p):
    return torch.zeros_like(p) if p.grad is None else p.grad.clone()


def _schnet_reference(loss):
    if loss not in _REF:
        b = _two_graphs()
        torch.manual_seed(3)
        ref = pbc_ref.PeriodicSchNet(**_C1)
        with torch.no_grad():
            ref.embedding.weight.normal_()
        state = copy.deepcopy(ref.state_dict())
        ref = ref.double()
        pos = b.pos.double().requires_grad_(True)
        E, F, sigma = pbc_ref.oracle_energy_forces_stress(
            ref, b.atoms, pos, b.cell.double(), b.edge_index, b.edge_shift_idx, b.batch,
            b.num_graphs, create_graph=True)
        _loss(E, F, sigma, [t.double() for t in _targets(b)], loss).backward()
        _REF[loss] = (state, E.detach(), F.detach(), sigma.detach(), pos.grad.clone(),
                      [_grad(p) for p in ref.parameters()])
    return _REF[loss]


@pytest.mark.parametrize("loss", ["force", "combined"])
def test_schnet_periodic_training_vs_oracle(loss):
    """SchNet C1 on two periodic graphs: E at 1e-5; F, sigma, and pos.grad and every parameter
    gradient of the force + stress loss (and the combined loss with |E - y|) within 1e-4 of
    scale of the fp64 periodic oracle."""
    import gmp_amd
    state, E64, F64, s64, pg64, grads64 = _schnet_reference(loss)
    b = _two_graphs().to(DEV)
    model = gmp_amd.SchNetModel(**_C1)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV)
    b.pos.requires_grad_(True)
    E, F, sigma = gmp_amd.energy_and_forces(model, b, stress=True)
    assert F.requires_grad and sigma.requires_grad and tuple(sigma.shape) == (2, 3, 3)
    _loss(E, F, sigma, [t.to(DEV) for t in _targets(b)], loss).backward()
    torch.testing.assert_close(E.detach().cpu().double(), E64, atol=1e-5, rtol=1e-5)
    _scaled(F, F64, 1e-4, "F")
    _scaled(sigma, s64, 1e-4, "sigma")
    _scaled(b.pos.grad, pg64, 1e-4, "pos.grad")
    for (k, p), q in zip(model.named_parameters(), grads64):
        _scaled(_grad(p), q, 1e-4, k)
    E2, F2 = gmp_amd.energy_and_forces(model, b, create_graph=False)  # stress=False: a pair
    assert not F2.requires_grad
    torch.testing.assert_close(E2, E.detach(), atol=1e-6, rtol=1e-6)
    _scaled(F2, F, 1e-6, "F without the strain")


@pytest.mark.parametrize("kind", ["mace", "tfn"])
def test_equivariant_periodic_first_order_vs_oracle(kind):
    """MACE (max_ell 2, correlation 3, 2 layers) and TFN on the two periodic graphs, first
    order: E at 1e-5 (+ the fp32 oracle's own rounding, as smoke() allows it); F and sigma
    within 1e-4 of scale of the fp64 oracle."""
    import gmp_amd
    b = _two_graphs()
    kw = dict(num_layers=2, emb_dim=16, r_max=3.0, mlp_dim=32, max_ell=2)
    if kind == "mace":
        kw["correlation"] = 3
        Ref, Model = om.MACEModel, gmp_amd.MACEModel
    else:
        kw["pool"] = "sum"
        Ref, Model = om.TFNModel, gmp_amd.TFNModel
    torch.manual_seed(1)
    ref = Ref(**kw)
    model = Model(**kw)
    model.load_state_dict(ref.state_dict())
    atoms = torch.zeros_like(b.atoms)  # in_dim = 1
    out = {}
    for name, r, dt in (("f32", ref, torch.float32), ("f64", copy.deepcopy(ref).double(),
                                                     torch.float64)):
        pos = b.pos.to(dt).requires_grad_(True)
        out[name] = [t.detach().double() for t in pbc_ref.oracle_energy_forces_stress(
            r, atoms, pos, b.cell.to(dt), b.edge_index, b.edge_shift_idx, b.batch, b.num_graphs,
            mace_like=True)]
    bd = b.to(DEV)
    bd.atoms = atoms.to(DEV)
    E, F, sigma = gmp_amd.energy_and_forces(model.to(DEV), bd, create_graph=False, stress=True)
    E64, F64, s64 = out["f64"]
    err32 = (out["f32"][0] - E64).abs().max().item()
    err = (E.cpu().double() - E64).abs().max().item()
    scale = max(1.0, E64.abs().max().item())
    print(f"E: {err:.3e} (fp32 oracle {err32:.3e}, scale {scale:.3e})")
    assert err <= 1e-5 * scale + 2 * err32
    _scaled(F, F64, 1e-4, "F")
    _scaled(sigma, s64, 1e-4, "sigma")


# ------------------------------------------------------------------------------------ properties
_BOX = 22.4


def _big(seed=5, n=2000):
    pos = pbc_ref.random_in_cell(n, np.eye(3) * _BOX, seed)
    atoms = torch.randint(1, 6, (n,), generator=torch.Generator().manual_seed(9))
    return torch.from_numpy(pos), atoms, torch.eye(3) * _BOX


def _big_model():
    import gmp_amd
    torch.manual_seed(21)
    return gmp_amd.SchNetModel(**dict(_C1, cutoff=3.0)).to(DEV)


def _periodic_batch(pos, atoms, cell, graph=None):
    """Batch on the device; the graph (cutoff 3 = the model's, so an edge that rounding moves
    across the cutoff carries no weight) is built there unless given."""
    import gmp_amd
    from gmp_amd.graph import Batch
    pos = pos.to(DEV)
    ei, S = graph if graph is not None else gmp_amd.radius_graph_pbc_gpu(pos, 3.0, cell)
    return Batch(atoms.to(DEV), pos, ei, num_graphs=1, cell=cell.view(1, 3, 3).to(DEV), pbc=ALL,
                 edge_shift_idx=S)


def test_periodic_forces_and_stress_rotate_sum_to_zero_and_are_symmetric():
    import gmp_amd
    pos, atoms, cell = _big()
    model = _big_model()
    b = _periodic_batch(pos, atoms, cell)
    assert 30000 < b.num_edges < 50000
    E, F, sigma = gmp_amd.energy_and_forces(model, b, create_graph=False, stress=True)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(2)).double())
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    q = q.float()
    br = _periodic_batch(pos @ q.t(), atoms, cell @ q.t(), (b.edge_index, b.edge_shift_idx))
    Er, Fr, sr = gmp_amd.energy_and_forces(model, br, create_graph=False, stress=True)
    torch.testing.assert_close(Er, E, atol=1e-5 * max(1.0, E.abs().max().item()), rtol=1e-5)
    _scaled(Fr, F.cpu() @ q.t(), 1e-4, "F(Rx) vs R F(x)")
    _scaled(sr[0], q @ sigma[0].cpu() @ q.t(), 1e-4, "sigma(Rx) vs R sigma R^T")
    scale = F.abs().max().item()
    tot = F.sum(0).abs().max().item()
    print(f"sum F = {tot:.3e}, scale {scale:.3e}")
    assert tot <= 1e-4 * scale
    _scaled(sigma[0], sigma[0].t(), 1e-4, "sigma vs sigma^T")


def test_periodic_energy_is_translation_invariant_with_the_graph_rebuilt():
    """All atoms moved by one vector, across cell faces (their wraps change), graph rebuilt."""
    pos, atoms, cell = _big()
    model = _big_model()
    with torch.no_grad():
        E0 = model(_periodic_batch(pos, atoms, cell))
        moved = pos + torch.tensor([7.3, -11.9, 30.1])
        E1 = model(_periodic_batch(moved, atoms, cell))
    print(f"E = {E0.item():.6f}, moved {E1.item():.6f}")
    torch.testing.assert_close(E1, E0, atol=1e-5 * max(1.0, E0.abs().max().item()), rtol=1e-5)


def test_periodic_force_step_is_bitwise_reproducible():
    """Two runs of the whole force + stress training step, graph build included, give bitwise
    equal graphs and parameter gradients."""
    import gmp_amd
    pos, atoms, cell = _big()
    model = _big_model()
    gen = torch.Generator().manual_seed(4)
    tg = [torch.randn(1, 1, generator=gen).to(DEV), torch.randn(len(pos), 3, generator=gen).to(DEV),
          torch.randn(1, 3, 3, generator=gen).to(DEV)]
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        b = _periodic_batch(pos, atoms, cell)
        E, F, sigma = gmp_amd.energy_and_forces(model, b, stress=True)
        _loss(E, F, sigma, tg, "combined").backward()
        runs.append([b.edge_index, b.edge_shift_idx, sigma.detach()]
                    + [p.grad.clone() for p in model.parameters()])
    for k, (x, y) in enumerate(zip(*runs)):
        assert torch.equal(x, y), k
