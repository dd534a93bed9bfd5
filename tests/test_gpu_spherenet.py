"""SphereNet on the GPU: K18 (spherical basis, fused triplet projections) and K19 (triplet
interaction) against the golden fp64 vectors of the reference (tests/golden/spherenet.pt, the
geometry held fixed) and, on shapes the golden does not hold, against the fp64 helper
tests/spherenet_ref.py (itself pinned to the golden by tests/test_spherenet_host.py)."""
import pytest
import torch

import spherenet_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("A", "B", "C")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("spherenet.pt")


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _bound(v64, err32):
    """The project's formula (__graft_entry__._check_vs_fp64): 1e-5 max(1, |v64|) + 2 err32."""
    return 1e-5 * max(1.0, _maxabs(v64)) + 2.0 * err32


def _check(name, got, want, bound):
    err = _maxabs(got.detach().cpu().double() - want)
    print(f"{name}: err {err:.3e} bound {bound:.3e} scale {_maxabs(want):.3e}")
    assert err <= bound, (name, err, bound)


def _check_scale(name, got, want):
    """1e-5 of the fp64 value's own scale; an identically zero reference must come out zero."""
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    scale = _maxabs(want)
    _check(name, got, want, 1e-5 * scale)


# ----------------------------------------------------------------------------------- basis
@pytest.mark.parametrize("case", CASES)
def test_basis_vs_golden(gold, case):
    import gmp_amd
    c = gold[case]
    kw, g, r64, e32 = c["kwargs"], c["geometry"], c["ref64"], c["err32"]
    emb = gmp_amd.emb(kw["num_spherical"], kw["num_radial"], c["cutoff"], 5).to(DEV)
    emb.dist_emb.freq.data.copy_(c["state_dict"]["emb.dist_emb.freq"])
    with torch.no_grad():
        rbf, a, t = emb.materialise(g["dist"].to(DEV), g["angle"].to(DEV), g["torsion"].to(DEV),
                                    g["idx_kj"].to(DEV))
    rows = c["emb_rows"]
    _check("dist_emb", rbf, r64["dist_emb"], _bound(r64["dist_emb"], e32["dist_emb"]))
    _check("angle_emb", a.cpu()[rows], r64["angle_emb"], _bound(r64["angle_emb"], e32["angle_emb"]))
    _check("torsion_emb", t.cpu()[rows], r64["torsion_emb"],
           _bound(r64["torsion_emb"], e32["torsion_emb"]))


def test_edge_basis_small_x(gold):
    """N_lq j_l(z_lq x) down to x = 0.01 against scipy's fp64 values, no allowance for the fp32
    reference: its closed forms give O(100) where the value is ~1e-11."""
    import gmp_amd
    sx = gold["small_x"]
    cutoff = 5.0
    emb = gmp_amd.emb(7, 6, cutoff, 5).to(DEV)
    dist = (sx["x"] * cutoff).float().to(DEV)
    with torch.no_grad():
        _, jb = emb(dist)
    want = sx["table"].reshape(-1, 42)
    # the table's x is exact, dist / cutoff in fp32 is not: the values move by l * 6e-8 relative
    _check("small-x jb", jb, want, 1e-5 * max(1.0, _maxabs(want)))
    rel = ((jb.cpu().double() - want).abs() / want.abs())[:-1]  # x = 1: the zeros themselves
    print("small-x worst relative error below x = 1:", float(rel.max()))


# ----------------------------------------------------------------------------------- model
def _load(c):
    import gmp_amd
    model = gmp_amd.SphereNetModel(cutoff=c["cutoff"], **c["kwargs"])
    model.load_state_dict(c["state_dict"], strict=True)
    return model.to(DEV)


@pytest.mark.parametrize("case", CASES)
def test_model_vs_golden(gold, case):
    c = gold[case]
    g, r64, e32 = c["geometry"], c["ref64"], c["err32"]
    model = _load(c)
    geo = [g[k].to(DEV).requires_grad_(True) for k in ("dist", "angle", "torsion")]
    G = int(c["batch"].max()) + 1
    out = model.forward_from_geometry(c["atoms"].to(DEV), geo[0], geo[1], geo[2], g["i"].to(DEV),
                                      g["j"].to(DEV), g["idx_kj"].to(DEV), g["idx_ji"].to(DEV),
                                      c["batch"].to(DEV), num_graphs=G)
    (out * c["w"].to(DEV)).sum().backward()
    scale = max(1.0, _maxabs(r64["out"]))
    _check("out", out, r64["out"], 1e-5 * scale + 2 * e32["out"])
    params = dict(model.named_parameters())
    assert sorted(k for k, p in params.items() if p.grad is None) == c["no_grad"]
    gmax = max(_maxabs(v) for v in c["grads64"].values())
    worst, wname = 0.0, ""
    for name, want in c["grads64"].items():
        den = max(_maxabs(want), 1e-3 * gmax)
        e = _maxabs(params[name].grad.detach().cpu().double() - want) / den
        if e > worst:
            worst, wname = e, name
    print(f"worst parameter gradient: {worst:.3e} ({wname})")
    assert worst <= 1e-4, (wname, worst)
    for t, name in zip(geo, ("g_dist", "g_angle", "g_torsion")):
        _check(name, t.grad, r64[name], _bound(r64[name], e32[name]))


# ----------------------------------------------------------------------------------- fused
def _graph(N, r, seed):
    """N points with pair distances >= 1, edges below r both ways, geometry from K11."""
    from gmp_amd.triplets import xyz_to_dat_offsets
    gen = torch.Generator().manual_seed(seed)
    pts = torch.zeros(0, 3)
    box = (N * 1.6) ** (1 / 3)
    while pts.shape[0] < N:
        p = torch.rand(1, 3, generator=gen) * box
        if pts.shape[0] == 0 or float((pts - p).norm(dim=1).min()) >= 1.0:
            pts = torch.cat([pts, p])
    d = (pts[:, None] - pts[None]).norm(dim=-1)
    src, dst = ((d < r) & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    ei = torch.stack([src, dst]).to(DEV)
    dist, angle, torsion, i, j, idx_kj, idx_ji, offs = xyz_to_dat_offsets(pts.to(DEV), ei, N)
    return dist, angle, torsion, idx_kj, idx_ji, offs


def _empty_geometry(E):
    """E edges of length 1.5 and no triplet (E = 2: two nodes and one edge pair; E = 0)."""
    f = dict(dtype=torch.float32, device=DEV)
    i64 = dict(dtype=torch.int64, device=DEV)
    return (torch.full((E,), 1.5, **f), torch.zeros(0, **f), torch.zeros(0, **f),
            torch.zeros(0, **i64), torch.zeros(0, **i64), torch.zeros(E + 1, **i64))


SHAPES = {
    "default": dict(N=40, I=64, n=7, k=6, ba=8, bt=8),
    "I6": dict(N=24, I=6, n=7, k=6, ba=8, bt=8),
    "I24": dict(N=24, I=24, n=3, k=2, ba=8, bt=8),
    "ba_ne_bt": dict(N=24, I=10, n=4, k=3, ba=5, bt=3),
    "n1": dict(N=24, I=8, n=1, k=6, ba=4, bt=4),
    "T0": dict(E=2, I=64, n=7, k=6, ba=8, bt=8),
    "E0": dict(E=0, I=64, n=7, k=6, ba=8, bt=8),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_vs_materialised(shape):
    from gmp_amd import ops
    from gmp_amd.spherenet import basis_tables
    s = SHAPES[shape]
    n, k, I, ba, bt, L, cutoff = s["n"], s["k"], s["I"], s["ba"], s["bt"], 2, 5.0
    if "N" in s:
        dist, angle, torsion, idx_kj, idx_ji, offs = _graph(s["N"], 2.0, 5)
    else:
        dist, angle, torsion, idx_kj, idx_ji, offs = _empty_geometry(s["E"])
    E, T = dist.numel(), angle.numel()
    print(f"{shape}: E {E} T {T}")
    gen = torch.Generator().manual_seed(7)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=gen, dtype=torch.float64) * sc)

    nk, nnk = n * k, n * n * k
    w64 = {"freq": torch.arange(1, k + 1, dtype=torch.float64) * torch.pi,
           "xd": rnd(E, I), "Wa": rnd(I, ba, sc=ba ** -0.5), "Wt": rnd(I, bt, sc=bt ** -0.5)}
    for l in range(L):
        w64[f"W1_{l}"] = rnd(ba, nk, sc=nk ** -0.5)
        w64[f"W2_{l}"] = rnd(bt, nnk, sc=nnk ** -0.5)
    cS, cP, cm = rnd(T, ba), rnd(T, bt), rnd(E, I)

    # ---- GPU, fused
    zeros, norm, pref = basis_tables(n, k)
    zt, nt = torch.from_numpy(zeros).to(DEV), torch.from_numpy(norm).to(DEV)
    pt = torch.from_numpy(pref).float().to(DEV)
    wg = {key: v.float().to(DEV).requires_grad_(True) for key, v in w64.items()}
    geo = [t.detach().clone().requires_grad_(True) for t in (dist, angle, torsion)]
    rbf, jb = ops.SphEdgeBasisFn.apply(geo[0], wg["freq"], zt, nt, cutoff, 5)
    weights = [wg[f"W1_{l}"] for l in range(L)] + [wg[f"W2_{l}"] for l in range(L)]
    SP = ops.SphTripletProjFn.apply(jb, geo[1], geo[2], idx_kj, pt, n, k, L, *weights)
    m = ops.TripletInteractFn.apply(wg["xd"], SP[1], SP[L + 1], wg["Wa"], wg["Wt"], idx_kj,
                                    idx_ji, offs)
    loss = (m * cm.float().to(DEV)).sum() + (SP[0] * cS.float().to(DEV)).sum() \
        + (SP[L] * cP.float().to(DEV)).sum() + rbf.sum()
    loss.backward()

    # ---- the fused projections against the materialised embeddings times the weights
    a_emb, t_emb = ops.sph_triplet_embeddings(jb.detach(), geo[1].detach(), geo[2].detach(),
                                              idx_kj, pt, n, k)
    assert tuple(a_emb.shape) == (T, nk) and tuple(t_emb.shape) == (T, nnk)
    for l in range(L):
        _check_scale(f"S[{l}] vs materialised", SP[l],
                     a_emb.cpu().double() @ w64[f"W1_{l}"].float().double().t())
        _check_scale(f"P[{l}] vs materialised", SP[L + l],
                     t_emb.cpu().double() @ w64[f"W2_{l}"].float().double().t())
    # ---- K19 against gather * product * index_add_ of its own inputs
    f64 = {key: v.float().double() for key, v in w64.items()}
    kj, ji = idx_kj.cpu(), idx_ji.cpu()
    _check_scale("m vs composed", m, ref.interact(f64["xd"], SP[1].detach().cpu().double(),
                                                  SP[L + 1].detach().cpu().double(), f64["Wa"],
                                                  f64["Wt"], kj, ji, E))

    # ---- everything against the fp64 helper, values and gradients
    r = {key: v.clone().requires_grad_(True) for key, v in f64.items()}
    rgeo = [t.detach().cpu().double().requires_grad_(True) for t in (dist, angle, torsion)]
    rrbf, rjb = ref.edge_basis(rgeo[0], r["freq"], n, k, cutoff)
    ra, rt = ref.triplet_embeddings(rjb, rgeo[1], rgeo[2], kj, n, k)
    rS = [ra @ r[f"W1_{l}"].t() for l in range(L)]
    rP = [rt @ r[f"W2_{l}"].t() for l in range(L)]
    rm = ref.interact(r["xd"], rS[1], rP[1], r["Wa"], r["Wt"], kj, ji, E)
    ((rm * cm.float().double()).sum() + (rS[0] * cS.float().double()).sum()
     + (rP[0] * cP.float().double()).sum() + rrbf.sum()).backward()
    _check_scale("rbf", rbf, rrbf.detach())
    _check_scale("jb", jb, rjb.detach())
    for l in range(L):
        _check_scale(f"S[{l}]", SP[l], rS[l].detach())
        _check_scale(f"P[{l}]", SP[L + l], rP[l].detach())
    _check_scale("m", m, rm.detach())
    for key in w64:
        want = r[key].grad if r[key].grad is not None else torch.zeros_like(r[key])
        _check_scale("grad " + key, wg[key].grad, want)
    for t, rt_, name in zip(geo, rgeo, ("dist", "angle", "torsion")):
        want = rt_.grad if rt_.grad is not None else torch.zeros_like(rt_)
        _check_scale("grad " + name, t.grad, want)


# ----------------------------------------------------------------------------------- end to end
def _batch(seed=3, N=30):
    from gmp_amd.graph import Batch
    gen = torch.Generator().manual_seed(seed)
    pts = torch.zeros(0, 3)
    while pts.shape[0] < N:
        p = torch.rand(1, 3, generator=gen) * 3.6
        if pts.shape[0] == 0 or float((pts - p).norm(dim=1).min()) >= 1.0:
            pts = torch.cat([pts, p])
    batch = (torch.arange(N) >= N // 2).long()
    d = (pts[:, None] - pts[None]).norm(dim=-1)
    same = batch[:, None] == batch[None]
    src, dst = ((d < 2.0) & same & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    atoms = torch.randint(1, 10, (N,), generator=gen)
    return Batch(atoms, pts, torch.stack([src, dst]), batch, num_graphs=2).to(DEV)


def _small_model(seed=0):
    import gmp_amd
    torch.manual_seed(seed)
    return gmp_amd.SphereNetModel(cutoff=5.0, num_layers=2, hidden_channels=16, int_emb_size=8,
                                  out_emb_channels=16, out_dim=1).to(DEV)


def test_end_to_end():
    import gmp_amd
    from gmp_amd.triplets import xyz_to_dat
    model, b = _small_model(), _batch()
    N = b.pos.shape[0]

    def run():
        model.zero_grad(set_to_none=True)
        pos = b.pos.detach().clone().requires_grad_(True)
        bb = gmp_amd.Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=2)
        out = model(bb)
        out.sum().backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        return out.detach(), pos.grad.clone(), grads

    out1, f1, g1 = run()
    out2, f2, g2 = run()
    assert torch.equal(out1, out2) and torch.equal(f1, f2)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1)

    with torch.no_grad():
        geom = xyz_to_dat(b.pos, b.edge_index, N, use_torsion=True)
        out3 = model.forward_from_geometry(b.atoms, *geom, b.batch, num_graphs=2)
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
    model, b = _small_model(1), _batch(4)
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
