"""DimeNet++ on periodic structures on the GPU (K11p, include/gmp.h): the image-aware triplet
enumeration against brute force, the vector-form geometry kernels and their second backward
against the fp64 closed forms of tests/dimenet_pbc_ref.py (pinned on the CPU by
tests/test_dimenet_pbc_host.py), and DimeNetPPModel(periodic=True): energy, forces and stress, and
training on them, against double autograd of the plain-torch helper.

Kernel-level bound: that of tests/test_gpu_dimenet_forces.py, 1e-5 of each array's scale against
fp64 on the same (fp32-rounded) vec; where an array misses it, plus twice the deviation of the
same closed form evaluated in fp32 on the CPU.  Model-level bounds: those of
test_model_force_training_vs_fp64 there.

Exactly collinear triplets (a self-image edge followed by the same self-image edge: v = 2u) keep
their angle in the comparison; their g_angle is zero (the chain through theta is 0 * inf there,
and kernels and reference alike drop the c^ terms), their number is the one known by construction
and below 5 % of T.
"""
import numpy as np
import pytest
import torch

import dimenet_pbc_ref as pref
import dimenet_ref as ref
import pbc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = (True, True, True)
CELL_1D = np.array([[1.7, 0, 0], [0, 9, 0], [0, 0, 9]], np.float32)
BIG = (np.eye(3) * 10).astype(np.float32)


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _check(name, got, want, bound):
    err = _maxabs(got.detach().cpu().double() - want)
    print(f"{name}: err {err:.3e} bound {bound:.3e} scale {_maxabs(want):.3e}")
    assert err <= bound, (name, err, bound)


def _check_kernel(name, got, want, want32=None):
    """1e-5 of the fp64 array's scale; if that is missed and the closed form's own fp32
    evaluation (want32, a callable) is given, plus twice that evaluation's deviation."""
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), name
    scale = _maxabs(want)
    err = _maxabs(got.detach().cpu().double() - want)
    bound = 1e-5 * scale
    if err > bound and want32 is not None:
        dev32 = _maxabs(want32().double() - want)
        print(f"{name}: fp32 closed form deviates by {dev32:.3e}")
        bound += 2.0 * dev32
    print(f"{name}: err {err:.3e} ({err / scale if scale else 0.0:.2e} of scale) bound {bound:.3e}")
    assert err <= bound, (name, err, bound)


def _spaced_in_cell(n, cell, seed, dmin=1.0):
    """n points in the cell, no two (images included) closer than dmin."""
    rng = np.random.default_rng(seed)
    c = np.asarray(cell, np.float64)
    imgs = np.array([[a, b, d] for a in range(-2, 3) for b in range(-2, 3)
                     for d in range(-2, 3)], np.float64) @ c
    pts = np.zeros((0, 3))
    while pts.shape[0] < n:
        p = rng.random(3) @ c
        d = np.linalg.norm(pts[:, None, :] - p[None, None, :] + imgs[None], axis=-1)
        if pts.shape[0] == 0 or d.min() >= dmin:
            pts = np.concatenate([pts, p[None]])
    return pts.astype(np.float32)


def _graph(pos, r, cell, pbc=ALL, batch=None):
    ei, S = pbc_ref.radius_graph_pbc(pos, r, cell, pbc, batch)
    return torch.from_numpy(ei), torch.from_numpy(S)


def _one_d():
    rng = np.random.default_rng(1)
    frac = rng.random((4, 3))
    frac[:, 1:] = 0.5 + 0.12 * (frac[:, 1:] - 0.5)
    pos = (frac @ CELL_1D.astype(np.float64)).astype(np.float32)
    return pos, CELL_1D, (True, False, False), 2.0


def _structure(name):
    """(pos (N, 3) fp32, cell (B, 3, 3), edge_index, shift_idx, batch) of a named case."""
    batch = None
    if name == "1d":
        pos, cell, pbc, r = _one_d()
    elif name == "thin12":
        pos, cell, pbc, r = pbc_ref.random_in_cell(12, pbc_ref.THIN, 3), pbc_ref.THIN, ALL, 2.0
    elif name == "one_atom":
        pos, cell, pbc, r = np.zeros((1, 3), np.float32), pbc_ref.CUBIC, ALL, 2.5
    elif name == "triclinic40":
        pos, cell, pbc, r = (pbc_ref.random_in_cell(40, pbc_ref.TRICLINIC, 4),
                             pbc_ref.TRICLINIC, ALL, 3.0)
    elif name == "slab":
        pos, cell, pbc, r = (pbc_ref.random_in_cell(12, pbc_ref.THIN, 5), pbc_ref.THIN,
                             (True, True, False), 2.5)
    elif name == "reverse_only":
        pos, cell, pbc, r = np.array([[1, 1, 1], [1.8, 1.3, 0.9]], np.float32), BIG, ALL, 1.5
    elif name == "no_edges":
        pos, cell, pbc, r = np.array([[1, 1, 1], [5, 5, 5]], np.float32), BIG, ALL, 1.5
    elif name == "two_graphs":
        pos = np.concatenate([pbc_ref.random_in_cell(7, pbc_ref.THIN, 6),
                              pbc_ref.random_in_cell(11, pbc_ref.TRICLINIC, 7)])
        cell = np.stack([pbc_ref.THIN, pbc_ref.TRICLINIC])
        batch = np.array([0] * 7 + [1] * 11)
        pbc, r = ALL, 2.5
    else:
        raise KeyError(name)
    ei, S = _graph(pos, r, cell, pbc, batch)
    batch = torch.zeros(len(pos), dtype=torch.long) if batch is None else torch.from_numpy(batch)
    return (torch.from_numpy(pos), torch.from_numpy(np.asarray(cell)).reshape(-1, 3, 3), ei, S,
            batch)


def _lists(N, ei, S):
    from gmp_amd import triplets
    out = triplets.dimenet_triplets(ei.to(DEV), N, S.to(DEV))
    return out[-2].cpu(), out[-1].cpu()


# ----------------------------------------------------------------------------- 1. enumeration
@pytest.mark.parametrize("name", ["1d", "thin12", "one_atom", "triclinic40", "slab",
                                  "two_graphs", "reverse_only", "no_edges"])
def test_enumeration(name):
    pos, cell, ei, S, batch = _structure(name)
    N, E = pos.shape[0], ei.shape[1]
    want_kj, want_ji = pref.triplets(ei, S)
    T = want_kj.numel()
    print(f"{name}: N {N} E {E} T {T}")
    row, col = ei
    n_self = int((row == col).sum())
    if name == "1d":
        assert (E, T, n_self) == (36, 290, 8)
    elif name == "thin12":
        # several images of the same neighbour, and an exclusion in the middle of a run
        key = (col * N + row).numpy()
        assert np.unique(key, return_counts=True)[1].max() >= 3
        inside = False
        for e in range(E):
            run = ((col == row[e]) & (row == col[e])).nonzero().flatten()
            rev = (S[run] == -S[e]).all(1).nonzero().flatten()
            inside |= run.numel() >= 3 and 0 < int(rev[0]) < run.numel() - 1
        assert inside
    elif name == "one_atom":
        assert (E, T, n_self) == (80, 80 * 79, 80)
    elif name == "triclinic40":
        assert E > 256 and n_self == 0
    elif name == "slab":
        assert bool((S[:, 2] == 0).all()) and bool((S[:, :2] != 0).any())
    elif name == "two_graphs":
        assert bool((batch[row] == batch[col]).all()) and int(batch[col].max()) == 1
    elif name == "reverse_only":
        assert (E, T) == (2, 0)
    elif name == "no_edges":
        assert (E, T) == (0, 0)
    got_kj, got_ji = _lists(N, ei, S)
    assert torch.equal(got_kj, want_kj) and torch.equal(got_ji, want_ji)
    assert bool((got_ji[1:] >= got_ji[:-1]).all())


def test_enumeration_of_a_collated_batch_and_of_the_device_builder():
    import gmp_amd
    from gmp_amd.graph import Batch, collate
    gs = []
    for k, (cell, n) in enumerate(((pbc_ref.THIN, 6), (pbc_ref.TRICLINIC, 10))):
        pos = pbc_ref.random_in_cell(n, cell, 30 + k)
        ei, S = _graph(pos, 2.5, cell)
        gs.append(Batch(torch.ones(n, dtype=torch.long), torch.from_numpy(pos), ei, num_graphs=1,
                        cell=torch.from_numpy(cell), pbc=ALL, edge_shift_idx=S))
    b = collate(gs)
    want = pref.triplets(b.edge_index, b.edge_shift_idx)
    got = _lists(b.pos.shape[0], b.edge_index, b.edge_shift_idx)
    assert want[0].numel() > 0 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the graph of the device builder
    pos = torch.from_numpy(pbc_ref.random_in_cell(12, pbc_ref.THIN, 3))
    ei, S = gmp_amd.radius_graph_pbc_gpu(pos.to(DEV), 2.0, torch.from_numpy(pbc_ref.THIN))
    ei, S = ei.cpu(), S.cpu()
    assert bool((ei[0] == ei[1]).any())
    want = pref.triplets(ei, S)
    got = _lists(12, ei, S)
    assert want[0].numel() > 0 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_enumeration_with_a_duplicated_edge():
    """The same (j, i, S) twice: as an edge it owns its own triplets, as an entry both copies are
    excluded from the triplets of the reverse image."""
    pos, cell, ei, S, _ = _structure("1d")
    dup = torch.tensor([0, 5, 17])
    ei, S = torch.cat([ei, ei[:, dup]], 1), torch.cat([S, S[dup]])
    want = pref.triplets(ei, S)
    got = _lists(pos.shape[0], ei, S)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    e = int(dup[0])
    rev = ((ei[0] == ei[1][e]) & (ei[1] == ei[0][e]) & (S == -S[e]).all(1)).nonzero().flatten()
    assert rev.numel() >= 1
    kj_of_rev = got[0][got[1] == rev[0]]
    assert e not in kj_of_rev and ei.shape[1] - 3 not in kj_of_rev


def test_zero_shifts_are_the_open_boundary_lists_and_dist():
    from gmp_amd import triplets
    gen = torch.Generator().manual_seed(2)
    pos = torch.rand(30, 3, generator=gen) * 3.6
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    src, dst = ((d < 2.0) & ~torch.eye(30, dtype=torch.bool)).nonzero(as_tuple=True)
    ei = torch.stack([src, dst]).to(DEV)
    E = ei.shape[1]
    assert E > 256
    p = pos.to(DEV)
    open_ = triplets.dimenet_angles(p, ei, 30)
    zero = triplets.dimenet_angles(p, ei, 30, shift=torch.zeros(E, 3, device=DEV),
                                   shift_idx=torch.zeros(E, 3, dtype=torch.int32, device=DEV))
    assert open_[-1].numel() > 0
    assert torch.equal(zero[-2], open_[-2]) and torch.equal(zero[-1], open_[-1])
    assert torch.equal(zero[0], open_[0])  # dist, bit for bit
    assert _maxabs(zero[1] - open_[1]) <= 1e-5  # u + (p_k - p_j) against p_k - p_i: rounding
    with pytest.raises(ValueError):
        triplets.dimenet_angles(p, ei, 30, shift=torch.zeros(E, 3, device=DEV))


# ----------------------------------------------------------------------------- 2. geometry kernels
def _device_vec(pos, cell, ei, S, batch):
    """vec (E, 3) on the device as the model forms it, and its fp64 copy."""
    from gmp_amd import ops, triplets
    shift = ops.edge_shift_vectors(S.to(DEV), cell.to(DEV), batch.to(DEV)[ei[1].to(DEV)])
    vec = triplets.edge_vectors(pos.to(DEV), ei.to(DEV), shift)
    return vec, vec.cpu().double()


def _kernel_case(name, use_d=True, use_a=True, on_collinear=False, seed=23):
    from gmp_amd import triplets
    pos, cell, ei, S, batch = _structure(name)
    N, E = pos.shape[0], ei.shape[1]
    vec, vec64 = _device_vec(pos, cell, ei, S, batch)
    dist, angle, idx_kj, idx_ji = triplets._run_pbc(vec, ei.to(DEV), N, S.to(DEV))
    kj, ji = idx_kj.cpu(), idx_ji.cpu()
    want_kj, want_ji = pref.triplets(ei, S)
    assert torch.equal(kj, want_kj) and torch.equal(ji, want_ji)
    T = kj.numel()
    coll = pref.collinear(vec64, kj, ji)
    by_construction = (kj == ji) & (ei[0] == ei[1])[ji] if T else coll
    assert torch.equal(coll, by_construction)
    assert torch.equal(pref.collinear(vec.cpu(), kj, ji), coll)  # in fp32 as in fp64: v = 2u
    print(f"{name}: E {E} T {T} collinear {int(coll.sum())}")
    assert int(coll.sum()) < 0.05 * max(T, 1) or T == 0
    gen = torch.Generator().manual_seed(seed)
    g_dist = torch.randn(E, generator=gen) if use_d else None
    g_angle = torch.randn(T, generator=gen) if use_a else None
    if use_a and not on_collinear:
        g_angle = g_angle * (~coll)
    a_vec = torch.randn(E, 3, generator=gen)
    v = vec.detach().requires_grad_(True)
    gd = g_dist.to(DEV).requires_grad_(True) if use_d else None
    ga = g_angle.to(DEV).requires_grad_(True) if use_a else None
    g_vec = triplets.TripletVecGeomBwdFn.apply(v, idx_kj, idx_ji, gd, ga)
    wrt = [t for t in (gd, ga, v) if t is not None]
    out = list(torch.autograd.grad((g_vec * a_vec.to(DEV)).sum(), wrt, create_graph=True))
    gg_d = out.pop(0) if use_d else None
    gg_a = out.pop(0) if use_a else None
    h_vec = out.pop(0)
    with pytest.raises(RuntimeError):  # exactly two orders
        h_vec.sum().backward()
    got = dict(dist=dist, angle=angle, g_vec=g_vec.detach(), gg_dist=gg_d, gg_angle=gg_a,
               h_vec=h_vec.detach())

    def closed(dtype):
        o = lambda t: None if t is None else t.to(dtype)  # noqa: E731
        x = vec64.to(dtype)
        d, a = pref.geometry_from_vec(x, kj, ji)
        g = pref.vec_bwd(x, kj, ji, o(g_dist), o(g_angle))
        ggd, gga, h = pref.vec_bwd2(x, kj, ji, o(g_dist), o(g_angle), a_vec.to(dtype))
        return dict(dist=d, angle=a, g_vec=g, gg_dist=ggd, gg_angle=gga, h_vec=h)

    return got, closed, coll


@pytest.mark.parametrize("cots", ["both", "g_dist", "g_angle"])
@pytest.mark.parametrize("name", ["thin12", "triclinic40", "1d"])
def test_geometry_kernels(name, cots):
    got, closed, coll = _kernel_case(name, cots != "g_angle", cots != "g_dist")
    want = closed(torch.float64)
    if name != "triclinic40":
        assert int(coll.sum()) > 0
    for key, g in got.items():
        if g is not None:
            _check_kernel(f"{key} [{name}, {cots}]", g, want[key],
                          lambda key=key: closed(torch.float32)[key])
    assert _maxabs(want["h_vec"]) > 0 and _maxabs(want["g_vec"]) > 0


def test_geometry_kernels_no_triplets():
    got, closed, _ = _kernel_case("reverse_only")
    want = closed(torch.float64)
    assert tuple(got["angle"].shape) == (0,) and tuple(got["gg_angle"].shape) == (0,)
    for key in ("dist", "g_vec", "gg_dist", "h_vec"):
        _check_kernel(key, got[key], want[key], lambda key=key: closed(torch.float32)[key])
    # no edge at all
    from gmp_amd import triplets
    i64 = dict(dtype=torch.int64, device=DEV)
    vec = torch.zeros(0, 3, device=DEV, requires_grad=True)
    out = triplets._geom_pbc(vec, torch.zeros(2, 0, **i64), 3,
                             torch.zeros(0, 3, dtype=torch.int32, device=DEV), twice=True)
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0,), (0,)]
    g = triplets.TripletVecGeomBwdFn.apply(vec, out[2], out[3], None, None)
    assert tuple(g.shape) == (0, 3)


def test_geometry_kernels_cotangent_on_collinear_triplets_stays_finite():
    got, _, coll = _kernel_case("1d", on_collinear=True)
    assert int(coll.sum()) == 8
    assert all(bool(torch.isfinite(t).all()) for t in got.values())


# ----------------------------------------------------------------------------- 3. / 4. the model
R = 3.0
WIDTHS = {
    "small": dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16, num_layers=2),
    "default": dict(hidden_channels=128, int_emb_size=64, basis_emb_size=8,
                    out_emb_channels=256, num_layers=2),
}
_CACHE = {}


def _batch_cpu():
    """TRICLINIC with 20 atoms and THIN (thinner than the cutoff) with 6, cutoff = r = 3."""
    if "batch" not in _CACHE:
        from gmp_amd.graph import Batch, collate
        gs = []
        for k, (cell, n) in enumerate(((pbc_ref.TRICLINIC, 20), (pbc_ref.THIN, 6))):
            pos = _spaced_in_cell(n, cell, 40 + k)
            ei, S = _graph(pos, R, cell)
            atoms = torch.randint(1, 10, (n,), generator=torch.Generator().manual_seed(k))
            gs.append(Batch(atoms, torch.from_numpy(pos), ei, num_graphs=1,
                            cell=torch.from_numpy(cell), pbc=ALL, edge_shift_idx=S))
        assert bool((gs[1].edge_index[0] == gs[1].edge_index[1]).any())  # self-image edges
        _CACHE["batch"] = collate(gs)
    return _CACHE["batch"]


def _state(kw, seed=0, **flags):
    """A DimeNetPPModel (on the CPU) with a seeded state dict and random
    output_blocks.*.lin.weight (PyG's zero initialisation zeroes nearly every gradient)."""
    import gmp_amd
    torch.manual_seed(seed)
    model = gmp_amd.DimeNetPPModel(cutoff=R, **kw, **flags)
    sd = {key: v.clone() for key, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 100)
    for key in sd:
        if key.startswith("output_blocks.") and key.endswith(".lin.weight"):
            w = sd[key]
            sd[key] = torch.randn(w.shape, generator=gen) * (2.0 / (w.shape[0] + w.shape[1])) ** 0.5
    model.load_state_dict(sd, strict=True)
    return model, sd


def _targets(b):
    gen = torch.Generator().manual_seed(17)
    return (torch.randn(2, 1, generator=gen), torch.randn(b.pos.shape[0], 3, generator=gen),
            torch.randn(2, 3, 3, generator=gen) * 0.01)


def _loss(kind, energy, forces, sigma, tg):
    y, f_star, s_star = tg
    loss = (forces - f_star).pow(2).sum() + (sigma - s_star).pow(2).sum()
    return loss + (energy - y).abs().sum() if kind == "energy+forces" else loss


def _reference_step(width, kind, dtype):
    """The step by autograd (create_graph=True) of the plain-torch helper on the CPU, under the
    symmetric strain of forces._strained: (E, F, sigma, pos.grad, parameter gradients)."""
    key = (width, kind, dtype)
    if key not in _CACHE:
        kw = WIDTHS[width]
        _, sd = _state(kw)
        b = _batch_cpu()
        sdt = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        pos = b.pos.detach().to(dtype).clone().requires_grad_(True)
        cell = b.cell.to(dtype)
        eps = torch.zeros(2, 3, 3, dtype=dtype, requires_grad=True)
        sym = 0.5 * (eps + eps.transpose(1, 2))
        p = pos + (pos.unsqueeze(2) * sym[b.batch]).sum(1)
        c = cell + (cell.unsqueeze(3) * sym.unsqueeze(1)).sum(2)
        dist, angle, i, j, kj, ji = pref.geometry(p, c, b.edge_index, b.edge_shift_idx.long(),
                                                  b.batch)
        energy = ref.model(sdt, dict(kw, cutoff=R), b.atoms, dist, angle, i, j, kj, ji, b.batch, 2)
        g, ge = torch.autograd.grad(energy.sum(), (pos, eps), create_graph=True)
        vol = torch.linalg.det(cell).abs().view(-1, 1, 1)
        sigma = ge / vol
        _loss(kind, energy, -g, sigma, [t.to(dtype) for t in _targets(b)]).backward()
        _CACHE[key] = (energy.detach().double(), -g.detach().double(), sigma.detach().double(),
                       pos.grad.double(), {k: (v.grad.double() if v.grad is not None else None)
                                           for k, v in sdt.items()})
    return _CACHE[key]


def _bound(v64, v32):
    return 1e-5 * max(1.0, _maxabs(v64)) + 2.0 * _maxabs(v32 - v64)


def _fresh(b):
    """The batch on the device with a fresh leaf pos."""
    bd = b.to(DEV)
    bd.pos = bd.pos.detach().clone().requires_grad_(True)
    return bd


@pytest.mark.parametrize("width", list(WIDTHS))
def test_model_first_order_vs_fp64(width):
    import gmp_amd
    model, _ = _state(WIDTHS[width], periodic=True)
    model = model.to(DEV).eval()
    b = _fresh(_batch_cpu())
    print(f"E {b.num_edges}")
    energy, forces, sigma = gmp_amd.energy_and_forces(model, b, stress=True)
    assert not forces.requires_grad and not sigma.requires_grad and b.pos.grad is None
    e64, f64, s64, _, _ = _reference_step(width, "forces", torch.float64)
    e32, f32, s32, _, _ = _reference_step(width, "forces", torch.float32)
    assert _maxabs(e64) > 0 and _maxabs(f64) > 0 and _maxabs(s64) > 0
    _check("E", energy, e64, _bound(e64, e32))
    _check("F", forces, f64, _bound(f64, f32))
    _check("sigma", sigma, s64, _bound(s64, s32))


def _force_step(model, b, kind):
    import gmp_amd
    model.zero_grad(set_to_none=True)
    bd = _fresh(b)
    energy, forces, sigma = gmp_amd.energy_and_forces(model, bd, stress=True)
    assert forces.requires_grad and sigma.requires_grad
    _loss(kind, energy, forces, sigma, [t.to(DEV) for t in _targets(b)]).backward()
    grads = {k: (p.grad.clone() if p.grad is not None else None)
             for k, p in model.named_parameters()}
    return energy.detach(), forces.detach(), sigma.detach(), bd.pos.grad.clone(), grads


@pytest.mark.parametrize("kind", ["forces", "energy+forces"])
@pytest.mark.parametrize("width", list(WIDTHS))
def test_model_force_training_vs_fp64(width, kind):
    model, _ = _state(WIDTHS[width], periodic=True, twice_differentiable=True)
    model = model.to(DEV).train()
    energy, forces, sigma, pos_grad, grads = _force_step(model, _batch_cpu(), kind)
    e64, f64, s64, p64, g64 = _reference_step(width, kind, torch.float64)
    e32, f32, s32, p32, g32 = _reference_step(width, kind, torch.float32)
    assert _maxabs(e64) > 0 and _maxabs(f64) > 0 and _maxabs(s64) > 0 and _maxabs(p64) > 0
    _check("E", energy, e64, _bound(e64, e32))
    _check("F", forces, f64, _bound(f64, f32))
    _check("sigma", sigma, s64, _bound(s64, s32))
    _check("pos.grad", pos_grad, p64, _bound(p64, p32))
    assert sorted(grads) == sorted(g64)
    if kind == "energy+forces":  # every parameter is reached
        zero = [k for k, v in g64.items() if v is None or _maxabs(v) == 0.0]
        assert zero == [], zero
    gmax = max(_maxabs(v) for v in g64.values() if v is not None)
    worst, wname = 0.0, ""
    for name, v in g64.items():
        if v is None:  # unreached in the reference (the energy's last bias under a force loss)
            assert grads[name] is None or _maxabs(grads[name]) == 0.0, name
            continue
        assert grads[name] is not None, name
        b_ = 1e-4 * max(_maxabs(v), 1e-3 * gmax) + 2.0 * _maxabs(g32[name] - v)
        e = _maxabs(grads[name].cpu().double() - v)
        if e / b_ > worst:
            worst, wname = e / b_, name
    print(f"worst parameter gradient: {worst:.3e} of its bound ({wname})")
    assert worst <= 1.0, (wname, worst)


# ----------------------------------------------------------------------------- 5. invariants
def test_net_force_is_zero_and_stress_is_symmetric():
    import gmp_amd
    model, _ = _state(WIDTHS["small"], periodic=True)
    model = model.to(DEV).eval()
    b = _fresh(_batch_cpu())
    _, forces, sigma = gmp_amd.energy_and_forces(model, b, stress=True)
    scale, N = _maxabs(forces), forces.shape[0]
    for g in range(2):
        tot = _maxabs(forces[b.batch == g].sum(0))
        print(f"graph {g}: sum F = {tot:.3e}, max |F| {scale:.3e}")
        assert tot <= 1e-4 * scale * N
    assert _maxabs(sigma) > 0
    assert _maxabs(sigma - sigma.transpose(1, 2)) <= 1e-4 * _maxabs(sigma)


def test_energy_is_unchanged_by_a_lattice_translation_of_one_atom():
    """One atom moved by a lattice vector of its cell, the graph rebuilt on the device."""
    import gmp_amd
    from gmp_amd.graph import Batch
    model, _ = _state(WIDTHS["small"], periodic=True)
    model = model.to(DEV).eval()
    b = _batch_cpu()
    e64 = _reference_step("small", "forces", torch.float64)[0]
    e32 = _reference_step("small", "forces", torch.float32)[0]

    def energy(pos):
        pos = pos.to(DEV)
        ei, S = gmp_amd.radius_graph_pbc_gpu(pos, R, b.cell, batch=b.batch.to(DEV), num_graphs=2)
        with torch.no_grad():
            return model(Batch(b.atoms.to(DEV), pos, ei, b.batch.to(DEV), num_graphs=2,
                               cell=b.cell.to(DEV), pbc=ALL, edge_shift_idx=S))

    e0 = energy(b.pos)
    moved = b.pos.clone()
    moved[3] += b.cell[0, 0] - b.cell[0, 2]
    moved[22] += 2 * b.cell[1, 0]
    e1 = energy(moved)
    _check("E (device graph) vs fp64", e0, e64, _bound(e64, e32))
    _check("E moved vs E", e1, e0.cpu().double(), _bound(e64, e32))


def test_force_steps_bit_identical():
    model, _ = _state(WIDTHS["small"], periodic=True, twice_differentiable=True)
    model = model.to(DEV).train()
    b = _batch_cpu()
    r1 = _force_step(model, b, "energy+forces")
    r2 = _force_step(model, b, "energy+forces")
    assert all(torch.equal(x, y) for x, y in zip(r1[:4], r2[:4]))
    assert r1[4].keys() == r2[4].keys() and all(torch.equal(r1[4][k], r2[4][k]) for k in r1[4])


def test_flag_on_without_shifts_is_the_open_boundary_model():
    import gmp_amd
    from gmp_amd.graph import Batch
    on, _ = _state(WIDTHS["small"], periodic=True)
    off, _ = _state(WIDTHS["small"])
    gen = torch.Generator().manual_seed(8)
    pos = torch.rand(24, 3, generator=gen) * 3.4
    batch = (torch.arange(24) >= 12).long()
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    ok = (d < 2.0) & (batch[:, None] == batch[None]) & ~torch.eye(24, dtype=torch.bool)
    ei = torch.stack(ok.nonzero(as_tuple=True))
    atoms = torch.randint(1, 10, (24,), generator=gen)
    out = []
    for model in (on, off):
        model = model.to(DEV).eval()
        p = pos.to(DEV).requires_grad_(True)
        bb = Batch(atoms.to(DEV), p, ei.to(DEV), batch.to(DEV), num_graphs=2)
        out.append(gmp_amd.energy_and_forces(model, bb))
    assert _maxabs(out[1][1]) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_flag_on_without_twice_is_once_differentiable():
    import gmp_amd
    model, _ = _state(WIDTHS["small"], periodic=True)
    model = model.to(DEV)
    b = _batch_cpu()
    energy, forces, sigma = gmp_amd.energy_and_forces(model.eval(), _fresh(b), stress=True)
    assert all(bool(torch.isfinite(t).all()) for t in (energy, forces, sigma))
    assert _maxabs(forces) > 0 and _maxabs(sigma) > 0
    energy, forces, sigma = gmp_amd.energy_and_forces(model.train(), _fresh(b), stress=True)
    with pytest.raises(RuntimeError):
        (forces.pow(2).sum() + sigma.pow(2).sum()).backward()
