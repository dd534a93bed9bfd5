"""DimeNet++ energy-and-force training on the GPU: the second backwards of K11 (triplet geometry),
K18d (edge basis, projection) and the composed K19d against the fp64 closed forms of
tests/dimenet_bwd2_ref.py (pinned to double autograd by tests/test_dimenet_forces_host.py), and
the model with twice_differentiable=True against double autograd of tests/dimenet_ref.py.

Kernel-level bound: the project's K18d / K19d bound, 1e-5 of each array's scale against fp64 on
the same (fp32-rounded) inputs.  Where an array misses it, the bound becomes 1e-5 of scale plus
twice the deviation of the same closed form evaluated in fp32 on the CPU; nothing else is added.
The 2^20 tile cap of the projection kernels and the grid-stride wrap of the geometry kernel need
more than 10^6 items and are not covered here.
"""
import pytest
import torch

import dimenet_bwd2_ref as ref2
import dimenet_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _opt(t, dtype):
    return None if t is None else t.to(dtype)


def _dev(t):
    return None if t is None else t.float().to(DEV)


def _points(N, seed, box=None):
    gen = torch.Generator().manual_seed(seed)
    pts = torch.zeros(0, 3)
    box = (N * 1.6) ** (1 / 3) if box is None else box
    while pts.shape[0] < N:
        p = torch.rand(1, 3, generator=gen) * box
        if pts.shape[0] == 0 or float((pts - p).norm(dim=1).min()) >= 1.0:
            pts = torch.cat([pts, p])
    return pts


def _radius_edges(pts, r):
    N = pts.shape[0]
    d = (pts[:, None] - pts[None]).norm(dim=-1)
    src, dst = ((d < r) & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    return torch.stack([src, dst])


def _tables(n, k):
    from gmp_amd.spherenet import basis_tables
    zeros, norm, pref = basis_tables(n, k)
    return (torch.from_numpy(zeros).to(DEV), torch.from_numpy(norm).to(DEV),
            torch.from_numpy(pref).float().to(DEV))


# ----------------------------------------------------------------------------- 1. geometry bwd2
def _triplets(pts, ei, mode):
    from gmp_amd import triplets
    _, _, _, idx_kj, idx_ji = triplets._run(pts.to(DEV), ei.to(DEV), pts.shape[0], mode, True,
                                            False, True)
    return idx_kj, idx_ji


def _geom_case(pts, ei, mode, use_d=True, use_a=True, seed=21):
    """TripletGeomBwdFn on the GPU and its second backward; returns the GPU results, the fp64
    closed form and a callable for the fp32 closed form."""
    from gmp_amd.triplets import TripletGeomBwdFn
    N, E = pts.shape[0], ei.shape[1]
    idx_kj, idx_ji = _triplets(pts, ei, mode)
    T = idx_kj.numel()
    print(f"mode {mode} N {N} E {E} T {T}")
    gen = torch.Generator().manual_seed(seed)
    g_dist = torch.randn(E, generator=gen) if use_d else None
    g_angle = torch.randn(T, generator=gen) if use_a else None
    a_pos = torch.randn(N, 3, generator=gen)
    pos = pts.to(DEV).requires_grad_(True)
    gd = g_dist.to(DEV).requires_grad_(True) if use_d else None
    ga = g_angle.to(DEV).requires_grad_(True) if use_a else None
    g_pos = TripletGeomBwdFn.apply(pos, ei.to(DEV), idx_kj, idx_ji, gd, ga, mode, N)
    wrt = [t for t in (gd, ga, pos) if t is not None]
    out = list(torch.autograd.grad((g_pos * a_pos.to(DEV)).sum(), wrt))
    gg_d = out.pop(0) if use_d else None
    gg_a = out.pop(0) if use_a else None
    h_pos = out.pop(0)
    pos2 = pts.to(DEV).requires_grad_(True)
    gp = TripletGeomBwdFn.apply(pos2, ei.to(DEV), idx_kj, idx_ji, gd, ga, mode, N)
    (h,) = torch.autograd.grad((gp * a_pos.to(DEV)).sum(), pos2, create_graph=True)
    with pytest.raises(RuntimeError):  # exactly two orders
        h.sum().backward()

    def closed(dtype):
        return ref2.geom_bwd2(pts.to(dtype), ei, idx_kj.cpu(), idx_ji.cpu(), mode,
                              _opt(g_dist, dtype), _opt(g_angle, dtype), a_pos.to(dtype))

    return (gg_d, gg_a, h_pos), closed(torch.float64), lambda: closed(torch.float32), idx_kj


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cots", ["both", "g_dist", "g_angle"])
def test_geometry_bwd2(mode, cots):
    pts = _points(40, 5)
    ei = _radius_edges(pts, 2.0)
    assert 100 <= ei.shape[1] <= 900
    got, want, want32, _ = _geom_case(pts, ei, mode, cots != "g_angle", cots != "g_dist")
    for i, name in enumerate(("gg_dist", "gg_angle", "h_pos")):
        if got[i] is not None:
            _check_kernel(f"{name} [{cots}]", got[i], want[i], lambda i=i: want32()[i])
    assert _maxabs(want[2]) > 0


@pytest.mark.parametrize("mode", [0, 1])
def test_geometry_bwd2_no_triplets(mode):
    # two atoms, an edge each way: E = 2, T = 0
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.1, 0.3, -0.4]])
    ei = torch.tensor([[0, 1], [1, 0]])
    got, want, _, idx_kj = _geom_case(pts, ei, mode)
    assert idx_kj.numel() == 0 and tuple(got[1].shape) == (0,)
    _check_kernel("gg_dist", got[0], want[0])
    _check_kernel("h_pos", got[2], want[2])
    # no edge at all
    from gmp_amd.triplets import TripletGeomBwdFn
    pos = torch.rand(3, 3).to(DEV).requires_grad_(True)
    i64 = dict(dtype=torch.int64, device=DEV)
    g_pos = TripletGeomBwdFn.apply(pos, torch.zeros(2, 0, **i64), torch.zeros(0, **i64),
                                   torch.zeros(0, **i64), None, None, mode, 3)
    assert tuple(g_pos.shape) == (3, 3) and _maxabs(g_pos.detach()) == 0.0
    (h,) = torch.autograd.grad(g_pos.sum(), pos)
    assert tuple(h.shape) == (3, 3) and _maxabs(h) == 0.0


@pytest.mark.parametrize("mode", [0, 1])
def test_geometry_bwd2_collinear(mode):
    """Atoms 0, 1, 2 on a line and one beside it: the triplets along the line are exactly
    collinear (b = 0).  Everything stays finite; the collinear triplets are left out of parity,
    and with them h_pos, which they reach."""
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [3.0, 0.0, 0.0], [1.5, 1.25, 0.5]])
    ei = _radius_edges(pts, 2.0)
    got, want, _, idx_kj = _geom_case(pts, ei, mode)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    _check_kernel("gg_dist", got[0], want[0])
    ok = torch.isfinite(want[1])
    idx_kj, idx_ji = _triplets(pts, ei, mode)
    row, col = ei
    e = idx_ji.cpu()
    on_line = (row[e] < 3) & (col[e] < 3) & (row[idx_kj.cpu()] < 3)
    assert int(on_line.sum()) >= 1 and int((~on_line).sum()) >= 1
    keep = ok & ~on_line
    _check_kernel("gg_angle (off the line)", got[1][keep.to(DEV)], want[1][keep])


# ----------------------------------------------------------------------------- 2. edge basis bwd2
def _edge_case(E, n, k, exponent, absent=None, x=None, seed=31):
    from gmp_amd import _lib
    cutoff = 5.0
    gen = torch.Generator().manual_seed(seed + E)
    if x is None:
        x = 0.01 + 0.989 * torch.rand(E, generator=gen)
        x[0] = 0.999
        if E > 1:
            x[1] = 0.01
    dist = (x * cutoff).float()
    freq = (torch.arange(1, k + 1) * torch.pi + 0.1 * torch.randn(k, generator=gen)).float()
    c = {"g_rbf": torch.randn(E, k, generator=gen), "g_sbe": torch.randn(E, n * k, generator=gen),
         "a_dist": torch.randn(E, generator=gen), "a_freq": torch.randn(k, generator=gen)}
    if absent:
        c[absent] = None
    zt, nt, _ = _tables(n, k)
    got = _lib.torch_ops().dime_edge_basis_bwd2(
        dist.to(DEV), freq.to(DEV), zt, nt, cutoff, exponent, _dev(c["g_rbf"]), _dev(c["g_sbe"]),
        _dev(c["a_dist"]), _dev(c["a_freq"]))

    def closed(dtype):
        return ref2.edge_basis_bwd2(dist.to(dtype), freq.to(dtype), n, k, cutoff, exponent,
                                    *[_opt(c[key], dtype) for key in
                                      ("g_rbf", "g_sbe", "a_dist", "a_freq")])

    return got, closed(torch.float64), lambda: closed(torch.float32), dist, cutoff


_EDGE_NAMES = ("gg_rbf", "gg_sbe", "h_dist", "h_freq")


@pytest.mark.parametrize("exponent", [5, 1])
@pytest.mark.parametrize("nk", [(7, 6), (3, 2)])
@pytest.mark.parametrize("E", [1, 257, 600])
def test_edge_basis_bwd2(E, nk, exponent):
    got, want, want32, _, _ = _edge_case(E, *nk, exponent)
    for i, name in enumerate(_EDGE_NAMES):
        _check_kernel(name, got[i], want[i], lambda i=i: want32()[i])


@pytest.mark.parametrize("absent", ["g_rbf", "g_sbe", "a_dist", "a_freq"])
def test_edge_basis_bwd2_absent(absent):
    got, want, want32, _, _ = _edge_case(257, 7, 6, 5, absent=absent)
    for i, name in enumerate(_EDGE_NAMES):
        _check_kernel(f"{name} [no {absent}]", got[i], want[i], lambda i=i: want32()[i])


@pytest.mark.parametrize("exponent", [5, 1])
def test_edge_basis_bwd2_cutoff(exponent):
    """Edges at the cutoff exactly and beyond: exact zeros in all four outputs, alone and mixed
    with live edges (whose values are unchanged by their dead neighbours)."""
    x = torch.tensor([1.0, 1.0 + 2.0 ** -20, 1.5, 40.0])
    got, _, _, dist, cutoff = _edge_case(4, 7, 6, exponent, x=x)
    assert bool((dist >= cutoff).all())
    for name, t in zip(_EDGE_NAMES, got):
        assert torch.equal(t, torch.zeros_like(t)), name
    x = torch.cat([torch.linspace(0.05, 0.95, 296), x])
    got, want, want32, dist, cutoff = _edge_case(300, 7, 6, exponent, x=x)
    dead = (dist >= cutoff).to(DEV)
    assert int(dead.sum()) == 4
    for name, t in zip(_EDGE_NAMES[:3], got[:3]):
        assert torch.equal(t[dead], torch.zeros_like(t[dead])), name
    for i, name in enumerate(_EDGE_NAMES):
        _check_kernel(name, got[i], want[i], lambda i=i: want32()[i])


# ----------------------------------------------------------------------------- 3. projection bwd2
def _proj_case(T, n, k, b, L, absent=None, hub=False, seed=41):
    from gmp_amd import _lib, ops
    E, nk = 23, n * k
    gen = torch.Generator().manual_seed(seed + T)

    def rnd(*sh):
        return torch.randn(*sh, generator=gen)

    sbe, W, gS = rnd(E, nk), rnd(L, b, nk) * nk ** -0.5, rnd(L, T, b)
    angle = 0.02 + 3.1 * torch.rand(T, generator=gen)
    if T >= 64:
        angle[0], angle[63] = 0.0, torch.pi
    idx_kj = torch.randint(0, E, (T,), generator=gen)
    if hub:
        idx_kj[torch.randperm(T, generator=gen)[:69]] = 3  # one edge gathered by >= 69 triplets
        assert int((idx_kj == 3).sum()) >= 69
    c = {"a_sbe": rnd(E, nk), "a_angle": rnd(T), "a_W": rnd(L, b, nk)}
    if absent:
        c[absent] = None
    _, _, pt = _tables(n, k)
    wt = ops.dime_feature_major(list(W.to(DEV)), nk)
    a_wt = None if c["a_W"] is None else ops.dime_feature_major(list(c["a_W"].to(DEV)), nk)
    kj = idx_kj.to(DEV)
    gg_S, h_wt, h_rows, h_angle = _lib.torch_ops().dime_triplet_proj_bwd2(
        sbe.to(DEV), angle.to(DEV), kj, pt, wt, n, k, L, b, gS.to(DEV), _dev(c["a_sbe"]),
        _dev(c["a_angle"]), a_wt, True)
    assert tuple(h_wt.shape) == tuple(wt.shape) and tuple(h_rows.shape) == (T, nk)
    assert _maxabs(h_wt[:, L * b:]) == 0.0  # the padding columns
    h_W = h_wt[:, :L * b].t().reshape(L, b, nk)
    h_sbe = ops._sum_rows_per_edge(h_rows, kj, sbe.to(DEV))

    def closed(dtype):
        return ref2.proj_bwd2(sbe.to(dtype), angle.to(dtype), idx_kj, n, k, W.to(dtype),
                              gS.to(dtype), *[_opt(c[key], dtype) for key in
                                              ("a_sbe", "a_angle", "a_W")])

    return (gg_S, h_W, h_sbe, h_angle), closed(torch.float64), lambda: closed(torch.float32)


_PROJ_NAMES = ("gg_S", "h_W", "h_sbe", "h_angle")


@pytest.mark.parametrize("bL", [(8, 1), (8, 3), (5, 1), (5, 3)])
@pytest.mark.parametrize("nk", [(7, 6), (3, 2), (2, 6)])
@pytest.mark.parametrize("T", [0, 1, 64, 65, 197])
def test_projection_bwd2(T, nk, bL):
    got, want, want32 = _proj_case(T, *nk, *bL, hub=T == 197)
    for i, name in enumerate(_PROJ_NAMES):
        _check_kernel(name, got[i], want[i], lambda i=i: want32()[i])
    if T == 0:
        assert all(_maxabs(t) == 0.0 for t in got)


@pytest.mark.parametrize("absent", ["a_sbe", "a_angle", "a_W"])
def test_projection_bwd2_absent(absent):
    got, want, want32 = _proj_case(197, 7, 6, 8, 3, absent=absent, hub=True)
    for i, name in enumerate(_PROJ_NAMES):
        _check_kernel(f"{name} [no {absent}]", got[i], want[i], lambda i=i: want32()[i])


# ----------------------------------------------------------------------------- 4. interaction
def _hub():
    """A centre with 70 leaves, edges both ways: each centre -> leaf edge owns 69 triplets."""
    from gmp_amd.triplets import dimenet_angles, triplet_offsets
    n_leaf = 70
    gen = torch.Generator().manual_seed(11)
    leaves = torch.randn(n_leaf, 3, generator=gen)
    leaves = 1.5 * leaves / leaves.norm(dim=1, keepdim=True)
    pts = torch.cat([torch.zeros(1, 3), leaves])
    idx = torch.arange(1, n_leaf + 1)
    z = torch.zeros(n_leaf, dtype=torch.long)
    ei = torch.stack([torch.cat([z, idx]), torch.cat([idx, z])])
    out = dimenet_angles(pts.to(DEV), ei.to(DEV), pts.shape[0])
    idx_kj, idx_ji = out[-2], out[-1]
    offs = triplet_offsets(idx_ji, ei.shape[1])
    assert int((offs[1:] - offs[:-1]).max()) == 69
    return ei.shape[1], idx_kj, idx_ji, offs


def _small_graph():
    from gmp_amd.triplets import dimenet_angles, triplet_offsets
    pts = _points(16, 9)
    ei = _radius_edges(pts, 2.0)
    out = dimenet_angles(pts.to(DEV), ei.to(DEV), pts.shape[0])
    idx_kj, idx_ji = out[-2], out[-1]
    return ei.shape[1], idx_kj, idx_ji, triplet_offsets(idx_ji, ei.shape[1])


def _no_triplets():
    i64 = dict(dtype=torch.int64, device=DEV)
    return 2, torch.zeros(0, **i64), torch.zeros(0, **i64), torch.zeros(3, **i64)


_INTERACT = {
    "I6_b5": (_small_graph, 6, 5), "I64_b8": (_small_graph, 64, 8),
    "I80_b16": (_small_graph, 80, 16), "I64_b5": (_small_graph, 64, 5),
    "I6_b16": (_small_graph, 6, 16), "hub": (_hub, 64, 8), "T0": (_no_triplets, 64, 8),
}


@pytest.mark.parametrize("case", list(_INTERACT))
def test_interaction_second_order_blocks(case):
    """The trilinear form F(gm, xd, S, W) of K19d: dF/d. through TripletInteract1_2Fn and every
    second-order block d(r_i . dF/di)/dj for all pairs i, j of gm, xd, S, W against fp64 autograd
    of gather * product * index_add_."""
    from gmp_amd import ops
    graph, I, b = _INTERACT[case]
    E, idx_kj, idx_ji, offs = graph()
    T = idx_kj.numel()
    print(f"E {E} T {T} I {I} b {b}")
    gen = torch.Generator().manual_seed(13)
    vals = [torch.randn(E, I, generator=gen), torch.randn(E, I, generator=gen),
            torch.randn(T, b, generator=gen), torch.randn(I, b, generator=gen) * b ** -0.5]
    cots = [torch.randn(v.shape, generator=gen) for v in vals]
    names = ("gm", "xd", "S", "W")
    r64 = [v.double().requires_grad_(True) for v in vals]
    gm, xd, S, W = r64
    F = (gm * ref.interact(xd, S, W, idx_kj.cpu(), idx_ji.cpu(), E)).sum()
    G64 = torch.autograd.grad(F, r64, create_graph=True)
    h = [v.to(DEV).requires_grad_(True) for v in vals]
    gm, xd, S, W = h
    m = ops.TripletInteract1_2Fn.apply(xd, S, W, idx_kj, idx_ji, offs)
    _check_kernel("m", m, G64[0].detach())
    Gh = torch.autograd.grad((gm * m).sum(), h, create_graph=True)
    for i in range(4):
        _check_kernel(f"dF/d{names[i]}", Gh[i], G64[i].detach())
        want = torch.autograd.grad((G64[i] * cots[i].double()).sum(), r64, retain_graph=True,
                                   allow_unused=True)
        got = torch.autograd.grad((Gh[i] * cots[i].to(DEV)).sum(), h, retain_graph=True,
                                  allow_unused=True)
        for j in range(4):
            wj = want[j] if want[j] is not None else torch.zeros_like(r64[j])
            gj = got[j] if got[j] is not None else torch.zeros_like(h[j])
            _check_kernel(f"d2F/d{names[i]}d{names[j]}", gj, wj.detach())


# ----------------------------------------------------------------------------- 5. model
def _batch_cpu(seed=3, N=30):
    from gmp_amd.graph import Batch
    gen = torch.Generator().manual_seed(seed)
    pts = _points(N, seed, box=3.6)
    batch = (torch.arange(N) >= N // 2).long()
    d = (pts[:, None] - pts[None]).norm(dim=-1)
    same = batch[:, None] == batch[None]
    src, dst = ((d < 2.0) & same & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    atoms = torch.randint(1, 10, (N,), generator=gen)
    return Batch(atoms, pts, torch.stack([src, dst]), batch, num_graphs=2)


def _batch(seed=3, N=30):
    return _batch_cpu(seed, N).to(DEV)


WIDTHS = {
    "small": dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16, num_layers=2),
    "default": dict(hidden_channels=128, int_emb_size=64, basis_emb_size=8,
                    out_emb_channels=256, num_layers=2),
}


def _state(kw, seed=0, twice=True):
    """A DimeNetPPModel (on the CPU) whose state dict is a seeded one with random
    output_blocks.*.lin.weight: with PyG's zero initialisation the output and nearly every
    gradient are identically zero."""
    import gmp_amd
    torch.manual_seed(seed)
    model = gmp_amd.DimeNetPPModel(cutoff=5.0, **kw, twice_differentiable=twice)
    sd = {key: v.clone() for key, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 100)
    for key in sd:
        if key.startswith("output_blocks.") and key.endswith(".lin.weight"):
            w = sd[key]
            sd[key] = torch.randn(w.shape, generator=gen) * (2.0 / (w.shape[0] + w.shape[1])) ** 0.5
    model.load_state_dict(sd, strict=True)
    return model, sd


def _model(kw, seed=0, twice=True):
    model, sd = _state(kw, seed, twice)
    return model.to(DEV), sd


def _targets(b):
    gen = torch.Generator().manual_seed(17)
    return torch.randn(2, 1, generator=gen), torch.randn(b.pos.shape[0], 3, generator=gen)


def _loss(kind, energy, forces, y, f_star):
    loss = (forces - f_star).pow(2).sum()
    return loss + (energy - y).abs().sum() if kind == "energy+forces" else loss


def _force_step(model, b, kind):
    """One energy-and-force training step on the GPU: (E, F, pos.grad, parameter gradients)."""
    import gmp_amd
    model.zero_grad(set_to_none=True)
    y, f_star = _targets(b)
    pos = b.pos.detach().clone().requires_grad_(True)
    bb = gmp_amd.Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=2)
    energy, forces = gmp_amd.energy_and_forces(model, bb)
    _loss(kind, energy, forces, y.to(DEV), f_star.to(DEV)).backward()
    grads = {k: (p.grad.clone() if p.grad is not None else None)
             for k, p in model.named_parameters()}
    return energy.detach(), forces.detach(), pos.grad.clone(), grads


_HELPER = {}


def _reference_step(width, kind, dtype):
    """The same step by autograd (create_graph=True) of the plain-torch helper, on the CPU."""
    key = (width, kind, dtype)
    if key not in _HELPER:
        kw = WIDTHS[width]
        _, sd = _state(kw)
        b = _batch_cpu()
        y, f_star = _targets(b)
        sdt = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        pos = b.pos.cpu().to(dtype).requires_grad_(True)
        dist, angle, i, j, idx_kj, idx_ji = ref.geometry(pos, b.edge_index.cpu())
        energy = ref.model(sdt, dict(kw, cutoff=5.0), b.atoms.cpu(), dist, angle, i, j, idx_kj,
                           idx_ji, b.batch.cpu(), 2)
        (g,) = torch.autograd.grad(energy.sum(), pos, create_graph=True)
        _loss(kind, energy, -g, y.to(dtype), f_star.to(dtype)).backward()
        _HELPER[key] = (energy.detach().double(), -g.detach().double(), pos.grad.double(),
                        {k: (v.grad.double() if v.grad is not None else None)
                         for k, v in sdt.items()})
    return _HELPER[key]


@pytest.mark.parametrize("kind", ["forces", "energy+forces"])
@pytest.mark.parametrize("width", list(WIDTHS))
def test_model_force_training_vs_fp64(width, kind):
    model, _ = _model(WIDTHS[width])
    model.train()
    energy, forces, pos_grad, grads = _force_step(model, _batch(), kind)
    e64, f64, p64, g64 = _reference_step(width, kind, torch.float64)
    e32, f32, p32, g32 = _reference_step(width, kind, torch.float32)

    def bound(v64, v32):
        return 1e-5 * max(1.0, _maxabs(v64)) + 2.0 * _maxabs(v32 - v64)

    assert _maxabs(e64) > 0 and _maxabs(f64) > 0 and _maxabs(p64) > 0
    _check("E", energy, e64, bound(e64, e32))
    _check("F", forces, f64, bound(f64, f32))
    _check("pos.grad", pos_grad, p64, bound(p64, p32))
    assert sorted(grads) == sorted(g64)
    if kind == "energy+forces":  # every parameter is reached, freq and every lin_sbf1 included
        zero = [k for k, v in g64.items() if v is None or _maxabs(v) == 0.0]
        assert zero == [], zero
        assert "rbf.freq" in g64 and sum(k.endswith("lin_sbf1.weight") for k in g64) == 2
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


def test_force_steps_bit_identical():
    model, _ = _model(WIDTHS["small"])
    model.train()
    b = _batch()
    e1, f1, p1, g1 = _force_step(model, b, "energy+forces")
    e2, f2, p2, g2 = _force_step(model, b, "energy+forces")
    assert torch.equal(e1, e2) and torch.equal(f1, f2) and torch.equal(p1, p2)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_flag_on_first_order_forces_match_flag_off():
    import gmp_amd
    on, _ = _model(WIDTHS["small"], twice=True)
    off, _ = _model(WIDTHS["small"], twice=False)
    on.eval(), off.eval()
    b = _batch()
    out = []
    for model in (on, off):
        pos = b.pos.detach().clone()
        bb = gmp_amd.Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=2)
        energy, forces = gmp_amd.energy_and_forces(model, bb)
        assert not forces.requires_grad and not energy.requires_grad
        assert pos.grad is None and all(p.grad is None for p in model.parameters())
        out.append((energy, forces))
    (e_on, f_on), (e_off, f_off) = out
    assert _maxabs(e_on - e_off) <= 1e-5 * _maxabs(e_off)
    assert _maxabs(f_off) > 0
    assert _maxabs(f_on - f_off) <= 1e-5 * _maxabs(f_off), _maxabs(f_on - f_off)


def test_orders_and_refusals():
    import gmp_amd
    model, _ = _model(WIDTHS["small"], seed=1)
    model.train()
    b = _batch(4)

    def fresh():
        pos = b.pos.detach().clone().requires_grad_(True)
        return pos, gmp_amd.Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=2)

    # flag on, outside second_order(): today's once-differentiable path
    pos, bb = fresh()
    (g,) = torch.autograd.grad(model(bb).sum(), pos, create_graph=True)
    with pytest.raises(RuntimeError):
        g.pow(2).sum().backward()
    # inside: two orders work, a third raises
    pos, bb = fresh()
    with gmp_amd.second_order():
        energy = model(bb)
    (g,) = torch.autograd.grad(energy.sum(), pos, create_graph=True)
    (h,) = torch.autograd.grad(g.pow(2).sum(), pos, create_graph=True)
    assert bool(torch.isfinite(h).all()) and _maxabs(h.detach()) > 0
    with pytest.raises(RuntimeError):
        h.pow(2).sum().backward()
    # periodic shifts are still refused
    pos, bb = fresh()
    bb.edge_shift_idx = torch.zeros(b.edge_index.shape[1], 3, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError), gmp_amd.second_order():
        model(bb)
    # the torsion has no second-order geometry
    from gmp_amd import triplets
    with pytest.raises(NotImplementedError):
        triplets._geom(pos, b.edge_index, pos.shape[0], 0, use_torsion=True, twice=True)
