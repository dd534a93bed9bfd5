"""Energy-and-force training for SchNet on the GPU (gmp_amd.second_order / energy_and_forces):
the three second-order kernels against fp64 torch autograd of the same formulas, the four
CFConv wrappers' second-order blocks, whole-model force losses against the fp64 oracle
(oracle/schnet.py), equivariance / determinism properties and the behaviour kept outside the
context.  Tolerances are the project's existing ones (tests/test_gpu_schnet.py): 1e-5 on
outputs, 1e-4 of scale (+ 1e-6) on gradients."""
import copy
import math

import pytest
import torch

from oracle import schnet as osch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _scaled(a, b, rtol, name):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    print(f"{name}: max|d|={err:.3e} scale={scale:.3e} ({err / scale:.2e} of scale)")
    assert err <= rtol * scale + 1e-6, f"{name}: max|d|={err:.3e} scale={scale:.3e}"


def _batches(kind):
    """tests/test_gpu_schnet.py::_batches, restated."""
    from gmp_amd.graph import collate, create_kchains, radius_graph
    if kind == "kchains":
        return collate(create_kchains(4))
    g = [radius_graph(num_nodes=200, target_edges=3000, r=3.0, seed=s, tol=0.2) for s in (1, 2)]
    for k, gg in enumerate(g):
        gg.atoms = torch.randint(0, 5, (gg.num_nodes,), generator=torch.Generator().manual_seed(k))
    return collate(g)


# ------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("F,n,E", [(128, 300, 5000), (4, 7, 40), (260, 33, 900), (64, 50, 0)])
def test_cfconv_cgrad_vs_fp64(F, n, E, scaled):
    """gmp_cfconv_cgrad_f32 against fp64 autograd of sum_e C_e sum_f g[gi] x[xi] w w.r.t. C."""
    from gmp_amd import ops
    gen = torch.Generator().manual_seed(F + n + E)
    gi, xi = torch.randint(0, n, (E,), generator=gen), torch.randint(0, n, (E,), generator=gen)
    g, x = torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen)
    w, es = torch.randn(E, F, generator=gen), torch.rand(E, generator=gen)
    dc, err = ops.cfconv_cgrad(g.to(DEV), gi.to(DEV), x.to(DEV), xi.to(DEV), w.to(DEV),
                               es.to(DEV) if scaled else None)
    assert tuple(dc.shape) == (E,) and int(err.item()) == 0
    if E == 0:
        return
    C = torch.ones(E, dtype=torch.float64, requires_grad=True)
    T = (C * (g.double()[gi] * x.double()[xi] * w.double()).sum(1)).sum()
    (ref,) = torch.autograd.grad(T, C)
    _scaled(dc, ref * es.double() if scaled else ref, 1e-4, "dC")


def test_cfconv_cgrad_out_of_range():
    """An out-of-range gather index contributes zero and sets the error flag."""
    from gmp_amd import ops
    F, n, E = 4, 7, 40
    gen = torch.Generator().manual_seed(5)
    gi, xi = torch.randint(0, n, (E,), generator=gen), torch.randint(0, n, (E,), generator=gen)
    g, x = torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen)
    w = torch.randn(E, F, generator=gen)
    ref = (g.double()[gi] * x.double()[xi] * w.double()).sum(1)
    gi[5], xi[9] = n, -1
    ref[5] = ref[9] = 0.0
    dc, err = ops.cfconv_cgrad(g.to(DEV), gi.to(DEV), x.to(DEV), xi.to(DEV), w.to(DEV))
    assert int(err.item()) != 0
    assert dc[5].item() == 0.0 and dc[9].item() == 0.0
    _scaled(dc, ref, 1e-4, "dC")


@pytest.mark.parametrize("n", [4, 4100])
def test_ssp_bwd2_vs_fp64(n):
    """gmp_ssp_bwd2_f32 against fp64 autograd of dx = g sigmoid(x), x spanning [-90, 90]; every
    output finite.  1e-5 relative + 1e-6 absolute."""
    from gmp_amd import _lib
    gen = torch.Generator().manual_seed(n)
    x = torch.linspace(-90.0, 90.0, n)
    g, a = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    gg, gx = _lib.torch_ops().ssp_bwd2(x.to(DEV), g.to(DEV), a.to(DEV))
    assert torch.isfinite(gg).all() and torch.isfinite(gx).all()
    xr, gr = x.double().requires_grad_(True), g.double().requires_grad_(True)
    rg, rx = torch.autograd.grad((gr * torch.sigmoid(xr) * a.double()).sum(), [gr, xr])
    torch.testing.assert_close(gg.cpu().double(), rg, atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(gx.cpu().double(), rx, atol=1e-6, rtol=1e-5)


def _featurize_bwd_ref(v, off, coeff, cutoff, g_d, g_rbf, g_cut):
    """The first-order backward g_vec = s(d) v / d in plain torch (any dtype), from vec."""
    d = v.norm(dim=-1)
    t = d[:, None] - off[None, :]
    dphi = torch.exp(coeff * t * t) * (2.0 * coeff * t)
    s = torch.zeros_like(d)
    if g_d is not None:
        s = s + g_d
    if g_rbf is not None:
        s = s + (g_rbf * dphi).sum(1)
    if g_cut is not None:
        s = s + g_cut * (-0.5 * (math.pi / cutoff) * torch.sin(d * math.pi / cutoff))
    return s[:, None] * v / d[:, None]


@pytest.mark.parametrize("E,G,cutoff,only_rbf", [(20000, 50, 10.0, False), (333, 7, 4.0, False),
                                                 (0, 50, 10.0, False), (333, 7, 4.0, True)])
def test_schnet_featurize_bwd2_vs_fp64(E, G, cutoff, only_rbf):
    """gmp_schnet_featurize_bwd2_f32 against fp64 autograd of the first-order backward formula.
    Edge 0 is a self-loop: exact zeros there, and it is left out of the autograd comparison
    (torch's second derivative of the norm at 0 is NaN).  only_rbf: every optional cotangent
    absent but g_rbf."""
    from gmp_amd import _lib
    gen = torch.Generator().manual_seed(E + G)
    n = max(E // 20, 4)
    pos = torch.rand(n, 3, generator=gen) * 1.5 * cutoff
    ei = torch.randint(0, n, (2, E), generator=gen)
    if E:
        ei[:, 0] = 3
    gs = osch.GaussianSmearing(0.0, cutoff, G)
    g_d, g_cut = torch.randn(E, generator=gen), torch.randn(E, generator=gen)
    g_rbf, a = torch.randn(E, G, generator=gen), torch.randn(E, 3, generator=gen)
    if only_rbf:
        g_d = g_cut = None
    dv = lambda t: None if t is None else t.to(DEV)
    out = _lib.torch_ops().schnet_featurize_bwd2(
        pos.to(DEV), ei.to(DEV), gs.offset.to(DEV), gs.coeff, cutoff, dv(g_d), dv(g_rbf),
        dv(g_cut), a.to(DEV), True, True, True, True)
    gg_d, gg_rbf, gg_cut, h = [t.cpu() for t in out]
    assert [tuple(t.shape) for t in (gg_d, gg_rbf, gg_cut, h)] == [(E,), (E, G), (E,), (E, 3)]
    if E == 0:
        return
    for t in (gg_d, gg_rbf, gg_cut, h):
        assert torch.isfinite(t).all()
        assert (t[0] == 0).all()  # the self-loop
    v = (pos.double()[ei[0]] - pos.double()[ei[1]])
    keep = v.norm(dim=-1) > 0
    assert not keep[0]
    f64 = lambda t: t.double()[keep].requires_grad_(True)
    v, rd, rr, rc = f64(v), f64(g_d if g_d is not None else torch.zeros(E)), f64(g_rbf), \
        f64(g_cut if g_cut is not None else torch.zeros(E))
    gv = _featurize_bwd_ref(v, gs.offset.double(), gs.coeff, cutoff, rd, rr, rc)
    refs = torch.autograd.grad((gv * a.double()[keep]).sum(), [rd, rr, rc, v])
    for got, ref, name in zip((gg_d, gg_rbf, gg_cut, h), refs, ("gg_d", "gg_rbf", "gg_cut", "h_vec")):
        _scaled(got[keep], ref, 1e-4, name)


def test_cfconv_wrappers_second_order_blocks():
    """The four CFConv wrappers (receiver / sender aggregate, edge product, edge dot) at
    (F, n, E) = (4, 7, 40): their values, and every second-order block d(r_i . dT/di)/dj for all
    pairs i, j of g, x, W, C, against fp64 autograd of the plain-torch expression
    scatter_add(x[src] * W * C[:, None])."""
    from gmp_amd import ops
    F, n, E = 4, 7, 40
    gen = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, E), generator=gen)
    src, dst = ei[0], ei[1]
    vals = [torch.randn(n, F, generator=gen), torch.randn(n, F, generator=gen),
            torch.randn(E, F, generator=gen), torch.rand(E, generator=gen)]
    cots = [torch.randn(v.shape, generator=gen) for v in vals]
    names = ("g", "x", "W", "C")

    r64 = [v.double().requires_grad_(True) for v in vals]
    g, x, W, C = r64
    T = (g * torch.zeros(n, F, dtype=torch.float64).index_add(
        0, dst, x[src] * W * C[:, None])).sum()
    G64 = torch.autograd.grad(T, r64, create_graph=True)

    h = [v.to(DEV).requires_grad_(True) for v in vals]
    g, x, W, C = h
    sd, dd = src.to(DEV), dst.to(DEV)
    direct = (ops.cfconv_receiver_aggregate(x, W, C, sd, dd, n),
              ops.cfconv_sender_aggregate(g, W, C, sd, dd, n),
              ops.cfconv_edge_product(g, x, C, sd, dd), ops.cfconv_edge_dot(g, x, W, sd, dd))
    for got, ref, nm in zip(direct, G64, names):
        _scaled(got, ref, 1e-4, f"dT/d{nm} (wrapper)")
    T = (g * ops.cfconv_receiver_aggregate(x, W, C, sd, dd, n)).sum()
    Gh = torch.autograd.grad(T, h, create_graph=True)
    for i in range(4):
        _scaled(Gh[i], G64[i], 1e-4, f"dT/d{names[i]}")
        ref = torch.autograd.grad((G64[i] * cots[i].double()).sum(), r64, retain_graph=True,
                                  allow_unused=True)
        got = torch.autograd.grad((Gh[i] * cots[i].to(DEV)).sum(), h, retain_graph=True,
                                  allow_unused=True)
        for j in range(4):
            rj = ref[j] if ref[j] is not None else torch.zeros_like(r64[j])
            gj = got[j] if got[j] is not None else torch.zeros_like(h[j])
            _scaled(gj, rj, 1e-4, f"d2T/d{names[i]}d{names[j]}")


# ------------------------------------------------------------------------------------ model
_C1 = dict(hidden_channels=64, num_filters=128, num_layers=4, num_gaussians=50, cutoff=10,
           out_dim=1)
_REF = {}


def _c1_models():
    torch.manual_seed(3)
    ref = osch.SchNetModel(**_C1)
    with torch.no_grad():  # atoms = 0 is the padding row: perturb so the test is not trivial
        ref.embedding.weight.normal_()
    return ref


def _targets(b):
    gen = torch.Generator().manual_seed(17)
    return (torch.randn(b.num_graphs, 1, generator=gen),
            torch.randn(b.pos.shape[0], 3, generator=gen))


def _loss(E, F, y, Fs, loss):
    lf = ((F - Fs) ** 2).sum()
    return lf if loss == "force" else (E - y).abs().sum() + lf


def _grad(p):
    """p.grad, zeros where the loss does not depend on p (lin2.bias under the force-only loss)."""
    return torch.zeros_like(p) if p.grad is None else p.grad.clone()


def _reference(kind, loss):
    """fp64 oracle: (state_dict, E, F, pos.grad, parameter gradients), computed once per case."""
    if (kind, loss) not in _REF:
        from gmp_amd.graph import Batch
        b = _batches(kind)
        ref = _c1_models()
        state = copy.deepcopy(ref.state_dict())
        ref = ref.double()
        y, Fs = _targets(b)
        pos = b.pos.double().requires_grad_(True)
        E = ref(Batch(b.atoms, pos, b.edge_index, b.batch, num_graphs=b.num_graphs))
        (g,) = torch.autograd.grad(E.sum(), pos, create_graph=True)
        _loss(E, -g, y.double(), Fs.double(), loss).backward()
        _REF[(kind, loss)] = (state, E.detach(), -g.detach(), pos.grad.clone(),
                              [_grad(p) for p in ref.parameters()])
    return _REF[(kind, loss)]


@pytest.mark.parametrize("loss", ["force", "combined"])
@pytest.mark.parametrize("edge_path", [False, True])
@pytest.mark.parametrize("kind", ["kchains", "radius"])
def test_schnet_force_training_vs_oracle(kind, edge_path, loss, monkeypatch):
    """Config C1 with out_dim = 1: E at 1e-5; F, pos.grad and every parameter gradient of the
    force-only loss sum (F - F*)^2 and the combined loss sum |E - y| + sum (F - F*)^2 within
    1e-4 of scale of the fp64 oracle.  edge_path: EDGE_LINEAR_MIN_ROWS = 1 sends the filter
    network through ops.linear's Functions.  Without the feature this fails with the
    once_differentiable RuntimeError (or an AttributeError on energy_and_forces)."""
    import gmp_amd
    from gmp_amd import ops
    from gmp_amd.graph import Batch
    if edge_path:
        monkeypatch.setattr(ops, "EDGE_LINEAR_MIN_ROWS", 1)
    state, E64, F64, pg64, grads64 = _reference(kind, loss)
    b = _batches(kind)
    y, Fs = _targets(b)
    model = gmp_amd.SchNetModel(**_C1)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV)
    pos = b.pos.to(DEV).requires_grad_(True)
    bd = Batch(b.atoms.to(DEV), pos, b.edge_index.to(DEV), b.batch.to(DEV),
               num_graphs=b.num_graphs)
    E, F = gmp_amd.energy_and_forces(model, bd)
    assert tuple(F.shape) == tuple(b.pos.shape) and F.requires_grad
    _loss(E, F, y.to(DEV), Fs.to(DEV), loss).backward()
    torch.testing.assert_close(E.detach().cpu().double(), E64, atol=1e-5, rtol=1e-5)
    _scaled(F, F64, 1e-4, "F")
    _scaled(pos.grad, pg64, 1e-4, "pos.grad")
    for (k, p), q in zip(model.named_parameters(), grads64):
        _scaled(_grad(p), q, 1e-4, k)


# ------------------------------------------------------------------------------------ properties
def _big_graph():
    from gmp_amd.graph import radius_graph
    g = radius_graph(num_nodes=2000, target_edges=40000, r=3.0, seed=5, tol=0.1)
    g.atoms = torch.randint(1, 6, (g.num_nodes,), generator=torch.Generator().manual_seed(9))
    return g


def _big_model():
    import gmp_amd
    torch.manual_seed(21)
    return gmp_amd.SchNetModel(**_C1).to(DEV)


def _forces(model, g, pos, create_graph=None):
    import gmp_amd
    from gmp_amd.graph import Batch
    batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    bd = Batch(g.atoms.to(DEV), pos, g.edge_index.to(DEV), batch, num_graphs=1)
    return gmp_amd.energy_and_forces(model, bd, create_graph=create_graph)


def test_forces_rotate_with_the_input_and_sum_to_zero():
    """F(R x) = R F(x) for a random rotation R (1e-4 of scale), and the per-graph sum of F
    vanishes (translation invariance, 1e-4 of the force scale)."""
    g, model = _big_graph(), _big_model()
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(2)).double())
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    q = q.float()
    _, F = _forces(model, g, g.pos.to(DEV), create_graph=False)
    _, Fr = _forces(model, g, (g.pos @ q.t()).to(DEV), create_graph=False)
    _scaled(Fr, F.cpu() @ q.t(), 1e-4, "F(Rx) vs R F(x)")
    scale = F.abs().max().item()
    tot = F.sum(0).abs().max().item()
    print(f"sum F = {tot:.3e}, scale {scale:.3e}")
    assert tot <= 1e-4 * scale


def test_force_step_is_bitwise_reproducible():
    """Two runs of the whole combined-loss step give bitwise-equal parameter gradients."""
    g, model = _big_graph(), _big_model()
    gen = torch.Generator().manual_seed(4)
    y, Fs = torch.randn(1, 1, generator=gen).to(DEV), torch.randn(g.num_nodes, 3,
                                                                  generator=gen).to(DEV)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        E, F = _forces(model, g, g.pos.to(DEV))
        _loss(E, F, y, Fs, "combined").backward()
        runs.append([p.grad.clone() for p in model.parameters()])
    for (k, _), a, b in zip(model.named_parameters(), *runs):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------ kept
def _small_step(model, b, ctx):
    from gmp_amd.graph import Batch
    pos = b.pos.to(DEV).requires_grad_(True)
    bd = Batch(b.atoms.to(DEV), pos, b.edge_index.to(DEV), b.batch.to(DEV),
               num_graphs=b.num_graphs)
    with ctx:
        E = model(bd)
    return E, pos


def test_outside_the_context_second_order_still_raises():
    import contextlib
    import gmp_amd
    b = _batches("radius")
    model = gmp_amd.SchNetModel(**_C1).to(DEV)
    E, pos = _small_step(model, b, contextlib.nullcontext())
    (g,) = torch.autograd.grad(E.sum(), pos, create_graph=True)
    with pytest.raises(RuntimeError):
        (g ** 2).sum().backward()


def test_egnn_inside_the_context_still_raises():
    """tests/test_gpu_egnn.py::test_double_backward_raises, run inside second_order()."""
    import gmp_amd
    from gmp_amd.graph import radius_graph
    torch.manual_seed(4)
    g = radius_graph(num_nodes=300, target_edges=4000, r=2.5, seed=6, shuffle=True)
    lay = gmp_amd.EGNNLayer(128, "relu", "layer", "sum").to(DEV)
    hd = torch.randn(g.num_nodes, 128, device=DEV, requires_grad=True)
    pd = g.pos.to(DEV).requires_grad_(True)
    with gmp_amd.second_order():
        ho, po = lay(hd, pd, g.edge_index.to(DEV))
        (gp,) = torch.autograd.grad(ho.sum() + po.sum(), [pd], create_graph=True)
        with pytest.raises(RuntimeError):
            gp.sum().backward()


def test_first_order_forces_match_outside_and_grads_untouched():
    """First-order forces inside the context equal those outside (1e-5 of scale), and
    energy_and_forces leaves every .grad as None."""
    import contextlib
    import gmp_amd
    from gmp_amd.graph import Batch
    b = _batches("radius")
    torch.manual_seed(8)
    model = gmp_amd.SchNetModel(**_C1).to(DEV)
    E0, pos0 = _small_step(model, b, contextlib.nullcontext())
    (g0,) = torch.autograd.grad(E0.sum(), pos0)
    pos = b.pos.to(DEV)
    bd = Batch(b.atoms.to(DEV), pos, b.edge_index.to(DEV), b.batch.to(DEV),
               num_graphs=b.num_graphs)
    E1, F1 = gmp_amd.energy_and_forces(model, bd)
    assert pos.requires_grad and pos.grad is None
    assert all(p.grad is None for p in model.parameters())
    torch.testing.assert_close(E1.detach(), E0.detach(), atol=1e-5, rtol=1e-5)
    _scaled(F1, -g0, 1e-5, "first-order F inside vs outside")
    model.eval()
    E2, F2 = gmp_amd.energy_and_forces(model, bd)
    assert not F2.requires_grad and not E2.requires_grad
    _scaled(F2, F1, 1e-6, "eval-mode F vs training-mode F")
