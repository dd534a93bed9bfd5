"""DimeNet++ on the GPU: K18d (angle-only spherical basis, fused triplet projections) and K19d
(one-factor triplet interaction) against the fp64 helper tests/dimenet_ref.py, whose basis
tests/test_dimenet_host.py pins to the golden vectors of the reference.  Structure, graph builder
and bounds are those of tests/test_gpu_spherenet.py."""
import pytest
import torch

import dimenet_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _check(name, got, want, bound):
    err = _maxabs(got.detach().cpu().double() - want)
    print(f"{name}: err {err:.3e} bound {bound:.3e} scale {_maxabs(want):.3e}")
    assert err <= bound, (name, err, bound)


def _check_scale(name, got, want):
    """1e-5 of the fp64 value's own scale; an identically zero reference must come out zero."""
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    _check(name, got, want, 1e-5 * _maxabs(want))


def _points(N, seed, box=None):
    gen = torch.Generator().manual_seed(seed)
    pts = torch.zeros(0, 3)
    box = (N * 1.6) ** (1 / 3) if box is None else box
    while pts.shape[0] < N:
        p = torch.rand(1, 3, generator=gen) * box
        if pts.shape[0] == 0 or float((pts - p).norm(dim=1).min()) >= 1.0:
            pts = torch.cat([pts, p])
    return pts


def _geometry(pts, ei):
    """dist, angle (vertex i), idx_kj, idx_ji, offsets from K11 (mode 1)."""
    from gmp_amd.triplets import dimenet_angles, triplet_offsets
    dist, angle, _, _, _, _, _, idx_kj, idx_ji = dimenet_angles(pts.to(DEV), ei.to(DEV),
                                                                 pts.shape[0])
    return dist, angle, idx_kj, idx_ji, triplet_offsets(idx_ji, dist.numel())


_GRAPHS = {}


def _graph(N, r=2.0, seed=5):
    """N points with pair distances >= 1, edges below r both ways, geometry from K11."""
    if (N, r, seed) not in _GRAPHS:
        pts = _points(N, seed)
        d = (pts[:, None] - pts[None]).norm(dim=-1)
        src, dst = ((d < r) & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
        _GRAPHS[(N, r, seed)] = _geometry(pts, torch.stack([src, dst]))
    return _GRAPHS[(N, r, seed)]


def _empty_geometry(E):
    """E edges of length 1.5 and no triplet (E = 2: two nodes and one edge pair; E = 0)."""
    f = dict(dtype=torch.float32, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    return (torch.full((E,), 1.5, **f), torch.zeros(0, **f), torch.zeros(0, **i64),
            torch.zeros(0, **i64), torch.zeros(E + 1, **i64))


def _tables(n, k):
    from gmp_amd.spherenet import basis_tables
    zeros, norm, pref = basis_tables(n, k)
    return (torch.from_numpy(zeros).to(DEV), torch.from_numpy(norm).to(DEV),
            torch.from_numpy(pref).float().to(DEV))


SHAPES = {
    "default": dict(N=40, I=64, n=7, k=6, b=8),
    "I6": dict(N=24, I=6, n=7, k=6, b=8),
    "I24": dict(N=24, I=24, n=3, k=2, b=8),
    "I80": dict(N=24, I=80, n=7, k=6, b=8),
    "b5": dict(N=24, I=10, n=4, k=3, b=5),
    "b16": dict(N=24, I=16, n=7, k=6, b=16),
    "n1": dict(N=24, I=8, n=1, k=6, b=4),
    "T0": dict(E=2, I=64, n=7, k=6, b=8),
    "E0": dict(E=0, I=64, n=7, k=6, b=8),
}


def _fused_case(geometry, n, k, I, b, cutoff, L=2):
    """The fused path (K18d edge basis -> K18d projections -> K19d) and the fp64 helper on the
    same inputs, loss touching m, S[0], S[1] and rbf; checks every value and gradient.  Returns
    what the callers look at further."""
    from gmp_amd import ops
    dist, angle, idx_kj, idx_ji, offs = geometry
    E, T = dist.numel(), angle.numel()
    print(f"E {E} T {T}")
    gen = torch.Generator().manual_seed(7)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=gen, dtype=torch.float64) * sc)

    nk = n * k
    w64 = {"freq": torch.arange(1, k + 1, dtype=torch.float64) * torch.pi,
           "xd": rnd(E, I), "W2": rnd(I, b, sc=b ** -0.5)}
    for l in range(L):
        w64[f"W1_{l}"] = rnd(b, nk, sc=nk ** -0.5)
    cS0, cS1, cm = rnd(T, b), rnd(T, b), rnd(E, I)

    # ---- GPU, fused
    zt, nt, pt = _tables(n, k)
    wg = {key: v.float().to(DEV).requires_grad_(True) for key, v in w64.items()}
    geo = [t.detach().clone().requires_grad_(True) for t in (dist, angle)]
    rbf, sbe = ops.DimeEdgeBasisFn.apply(geo[0], wg["freq"], zt, nt, cutoff, 5)
    S = ops.DimeTripletProjFn.apply(sbe, geo[1], idx_kj, pt, n, k, L,
                                    *[wg[f"W1_{l}"] for l in range(L)])
    m = ops.TripletInteract1Fn.apply(wg["xd"], S[1], wg["W2"], idx_kj, idx_ji, offs)
    loss = (m * cm.float().to(DEV)).sum() + (S[0] * cS0.float().to(DEV)).sum() \
        + (S[1] * cS1.float().to(DEV)).sum() + rbf.sum()
    loss.backward()

    # ---- the fused projections against the materialised embedding times the weights
    sbf = ops.dime_triplet_embeddings(sbe.detach(), geo[1].detach(), idx_kj, pt, n, k)
    assert tuple(sbf.shape) == (T, nk)
    for l in range(L):
        _check_scale(f"S[{l}] vs materialised", S[l],
                     sbf.cpu().double() @ w64[f"W1_{l}"].float().double().t())
    # ---- K19d against gather * product * index_add_ of its own inputs
    f64 = {key: v.float().double() for key, v in w64.items()}
    kj, ji = idx_kj.cpu(), idx_ji.cpu()
    _check_scale("m vs composed", m,
                 ref.interact(f64["xd"], S[1].detach().cpu().double(), f64["W2"], kj, ji, E))

    # ---- everything against the fp64 helper, values and gradients
    r = {key: v.clone().requires_grad_(True) for key, v in f64.items()}
    rgeo = [t.detach().cpu().double().requires_grad_(True) for t in (dist, angle)]
    rrbf, rsbe = ref.edge_basis(rgeo[0], r["freq"], n, k, cutoff)
    rsbf = ref.triplet_embedding(rsbe, rgeo[1], kj, n, k)
    rS = [rsbf @ r[f"W1_{l}"].t() for l in range(L)]
    rm = ref.interact(r["xd"], rS[1], r["W2"], kj, ji, E)
    ((rm * cm.float().double()).sum() + (rS[0] * cS0.float().double()).sum()
     + (rS[1] * cS1.float().double()).sum() + rrbf.sum()).backward()
    _check_scale("rbf", rbf, rrbf.detach())
    _check_scale("sbe", sbe, rsbe.detach())
    _check_scale("sbf", sbf, rsbf.detach())
    for l in range(L):
        _check_scale(f"S[{l}]", S[l], rS[l].detach())
    _check_scale("m", m, rm.detach())
    for key in w64:
        want = r[key].grad if r[key].grad is not None else torch.zeros_like(r[key])
        _check_scale("grad " + key, wg[key].grad, want)
    for t, rt_, name in zip(geo, rgeo, ("dist", "angle")):
        want = rt_.grad if rt_.grad is not None else torch.zeros_like(rt_)
        _check_scale("grad " + name, t.grad, want)
    return dict(rbf=rbf.detach(), sbe=sbe.detach(), sbf=sbf, g_dist=geo[0].grad, idx_kj=idx_kj)


# ----------------------------------------------------------------------------------- 1. fused
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_vs_materialised(shape):
    s = SHAPES[shape]
    geometry = _graph(s["N"]) if "N" in s else _empty_geometry(s["E"])
    _fused_case(geometry, s["n"], s["k"], s["I"], s["b"], cutoff=5.0)


# ----------------------------------------------------------------------------------- 2. cutoff
def test_cutoff_mask():
    geometry = _graph(40)
    dist = geometry[0]
    cutoff = 1.5
    beyond = dist >= cutoff
    assert bool(beyond.any()) and bool((~beyond).any())
    assert float(dist.min()) >= 1.0 and float(dist.max()) < 2.0
    out = _fused_case(geometry, 7, 6, 64, 8, cutoff=cutoff)
    assert float(out["rbf"][beyond].abs().max()) == 0.0
    assert float(out["sbe"][beyond].abs().max()) == 0.0
    assert float(out["g_dist"][beyond].abs().max()) == 0.0
    cut_triplets = beyond[out["idx_kj"]]
    assert bool(cut_triplets.any()) and bool((~cut_triplets).any())
    assert float(out["sbf"][cut_triplets].abs().max()) == 0.0
    assert float(out["sbf"][~cut_triplets].abs().max()) > 0.0
    assert float(out["g_dist"][~beyond].abs().max()) > 0.0


# ----------------------------------------------------------------------------------- 3. hub
def test_hub():
    """A centre with 70 leaves, edges both ways: each centre -> leaf edge owns 69 triplets (past
    one 64-triplet index batch of K19d's gradient kernel), the leaf -> centre edges none."""
    from gmp_amd import ops
    n_leaf, I, b = 70, 64, 8
    gen = torch.Generator().manual_seed(11)
    leaves = torch.randn(n_leaf, 3, generator=gen)
    leaves = 1.5 * leaves / leaves.norm(dim=1, keepdim=True)
    pts = torch.cat([torch.zeros(1, 3), leaves])
    idx = torch.arange(1, n_leaf + 1)
    ei = torch.stack([torch.cat([torch.zeros(n_leaf, dtype=torch.long), idx]),
                      torch.cat([idx, torch.zeros(n_leaf, dtype=torch.long)])])
    dist, angle, idx_kj, idx_ji, offs = _geometry(pts, ei)
    E, T = dist.numel(), angle.numel()
    counts = (offs[1:] - offs[:-1]).cpu()
    assert E == 2 * n_leaf and T == n_leaf * (n_leaf - 1)
    assert sorted(counts.tolist()) == [0] * n_leaf + [n_leaf - 1] * n_leaf

    def rnd(*sh):
        return torch.randn(*sh, generator=gen, dtype=torch.float64)

    w64 = {"xd": rnd(E, I), "S": rnd(T, b), "W": rnd(I, b) * b ** -0.5}
    cm = rnd(E, I).float()
    wg = {key: v.float().to(DEV).requires_grad_(True) for key, v in w64.items()}
    m = ops.TripletInteract1Fn.apply(wg["xd"], wg["S"], wg["W"], idx_kj, idx_ji, offs)
    (m * cm.to(DEV)).sum().backward()
    r = {key: v.float().double().requires_grad_(True) for key, v in w64.items()}
    rm = ref.interact(r["xd"], r["S"], r["W"], idx_kj.cpu(), idx_ji.cpu(), E)
    (rm * cm.double()).sum().backward()
    _check_scale("m", m, rm.detach())
    for key in w64:
        _check_scale("grad " + key, wg[key].grad, r[key].grad)


# ----------------------------------------------------------------------------------- 4. model
def _batch(seed=3, N=30):
    from gmp_amd.graph import Batch
    gen = torch.Generator().manual_seed(seed)
    pts = _points(N, seed, box=3.6)
    batch = (torch.arange(N) >= N // 2).long()
    d = (pts[:, None] - pts[None]).norm(dim=-1)
    same = batch[:, None] == batch[None]
    src, dst = ((d < 2.0) & same & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    atoms = torch.randint(1, 10, (N,), generator=gen)
    return Batch(atoms, pts, torch.stack([src, dst]), batch, num_graphs=2).to(DEV)


WIDTHS = {
    "small": dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16, num_layers=2),
    "default": dict(hidden_channels=128, int_emb_size=64, basis_emb_size=8,
                    out_emb_channels=256, num_layers=2),
}


def _model(kw, seed=0):
    """A DimeNetPPModel whose state dict is a seeded one with random output_blocks.*.lin.weight:
    with PyG's zero initialisation the output and nearly every gradient are identically zero."""
    import gmp_amd
    torch.manual_seed(seed)
    model = gmp_amd.DimeNetPPModel(cutoff=5.0, **kw)
    sd = {key: v.clone() for key, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 100)
    for key in sd:
        if key.startswith("output_blocks.") and key.endswith(".lin.weight"):
            w = sd[key]
            sd[key] = torch.randn(w.shape, generator=gen) * (2.0 / (w.shape[0] + w.shape[1])) ** 0.5
    model.load_state_dict(sd, strict=True)
    return model.to(DEV), sd


@pytest.mark.parametrize("width", list(WIDTHS))
def test_model_vs_fp64(width):
    from gmp_amd.triplets import dimenet_angles
    kw = WIDTHS[width]
    model, sd = _model(kw)
    b = _batch()
    N = b.pos.shape[0]
    with torch.no_grad():
        dist, angle, i, j, _, _, _, idx_kj, idx_ji = dimenet_angles(b.pos, b.edge_index, N)
    geo = [t.detach().clone().requires_grad_(True) for t in (dist, angle)]
    out = model.forward_from_geometry(b.atoms, geo[0], geo[1], i, j, idx_kj, idx_ji, b.batch,
                                      num_graphs=2)
    w = torch.tensor([[1.0], [-0.7]])
    (out * w.to(DEV)).sum().backward()

    def helper(dtype):
        sdt = {key: v.to(dtype).requires_grad_(True) for key, v in sd.items()}
        g = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (dist, angle)]
        o = ref.model(sdt, dict(kw, cutoff=5.0), b.atoms.cpu(), g[0], g[1], i.cpu(), j.cpu(),
                      idx_kj.cpu(), idx_ji.cpu(), b.batch.cpu(), 2)
        (o * w.to(dtype)).sum().backward()
        return o.detach().double(), sdt, [t.grad.double() for t in g]

    o64, sd64, g64 = helper(torch.float64)
    o32, _, g32 = helper(torch.float32)

    def bound(v64, v32):
        return 1e-5 * max(1.0, _maxabs(v64)) + 2.0 * _maxabs(v32 - v64)

    assert _maxabs(o64) > 0
    _check("out", out, o64, bound(o64, o32))
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(sd64)
    assert [k for k, p in params.items() if p.grad is None] == []
    gmax = max(_maxabs(v.grad) for v in sd64.values())
    worst, wname = 0.0, ""
    for name, v in sd64.items():
        assert v.grad is not None and _maxabs(v.grad) > 0, name
        den = max(_maxabs(v.grad), 1e-3 * gmax)
        e = _maxabs(params[name].grad.detach().cpu().double() - v.grad) / den
        if e > worst:
            worst, wname = e, name
    print(f"worst parameter gradient: {worst:.3e} ({wname})")
    assert worst <= 1e-4, (wname, worst)
    for t, want, w32, name in zip(geo, g64, g32, ("g_dist", "g_angle")):
        _check(name, t.grad, want, bound(want, w32))


# ----------------------------------------------------------------------------------- 5. end to end
def test_end_to_end():
    import gmp_amd
    from gmp_amd.triplets import dimenet_angles
    model, _ = _model(WIDTHS["small"])
    b = _batch()
    N = b.pos.shape[0]

    def run():
        model.zero_grad(set_to_none=True)
        pos = b.pos.detach().clone().requires_grad_(True)
        bb = gmp_amd.Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=2)
        out = model(bb)
        out.sum().backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters()}
        return out.detach(), pos.grad.clone(), grads

    out1, f1, g1 = run()
    out2, f2, g2 = run()
    assert torch.equal(out1, out2) and torch.equal(f1, f2)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)

    with torch.no_grad():
        dist, angle, i, j, _, _, _, idx_kj, idx_ji = dimenet_angles(b.pos, b.edge_index, N)
        out3 = model.forward_from_geometry(b.atoms, dist, angle, i, j, idx_kj, idx_ji, b.batch,
                                           num_graphs=2)
    assert torch.equal(out1, out3)

    assert bool(torch.isfinite(f1).all()) and _maxabs(f1) > 0
    # translation and rotation invariance: no net force, no net torque
    tol = 1e-4 * _maxabs(f1) * N
    F, pos = f1.double(), b.pos.double()
    torque = torch.linalg.cross(pos - pos.mean(0), F).sum(0)
    print("net force", F.sum(0).tolist(), "net torque", torque.tolist(), "tol", tol)
    assert _maxabs(F.sum(0)) <= tol, ("net force", F.sum(0), tol)
    assert _maxabs(torque) <= tol, ("net torque", torque, tol)


def test_second_order_raises_and_forces_api():
    import gmp_amd
    from gmp_amd import _lib
    model, _ = _model(WIDTHS["small"], seed=1)
    b = _batch(4)
    pos = b.pos.detach().clone().requires_grad_(True)
    bb = gmp_amd.Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=2)
    (g,) = torch.autograd.grad(model(bb).sum(), pos, create_graph=True)
    with pytest.raises(RuntimeError):
        g.pow(2).sum().backward()
    model.eval()
    energy, forces = gmp_amd.energy_and_forces(model, bb)
    assert tuple(energy.shape) == (2, 1) and tuple(forces.shape) == tuple(pos.shape)
    assert not forces.requires_grad and bool(torch.isfinite(forces).all())
    model.train()
    energy, forces = gmp_amd.energy_and_forces(model, bb)
    with pytest.raises(RuntimeError):
        (energy.sum() + forces.pow(2).sum()).backward()
    bb.edge_shift_idx = torch.zeros(b.edge_index.shape[1], 3, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError):
        model(bb)
    cpu = gmp_amd.Batch(b.atoms.cpu(), b.pos.cpu(), b.edge_index.cpu(), b.batch.cpu(),
                        num_graphs=2)
    with pytest.raises(_lib.GmpError):
        model(cpu)
