"""GPU parity of the GVP-GNN path (gmp_amd/gvp.py: split node projections + HIP gathers +
segmented mean) against the reference's own golden vectors (tests/golden/gvp_*.pt, eval mode)
and against the CPU oracle (oracle/gvp.py) at the C3 widths.  Tolerance: fp32 features within
1e-5; gradients within 1e-4 of their scale."""
import copy

import pytest
import torch

from oracle import gvp as ogvp

pytestmark = pytest.mark.gpu
DEV = "cuda"
RELU = torch.nn.functional.relu


def _scaled(a, b, rtol, name):
    a, b = a.detach().cpu(), b.detach().cpu()
    scale = b.abs().max().item() + 1e-6
    err = (a - b).abs().max().item()
    assert err <= rtol * scale + 1e-6, f"{name}: max|d|={err:.3e} scale={scale:.3e}"


def _params(d):
    return {k[6:]: v for k, v in d.items() if k.startswith("param.")}


def test_gvp_layer_golden(golden):
    import gmp_amd.gvp as g
    d = golden("gvp_layer.pt")
    layer = g.GVPConvLayer((32, 4), (8, 1), activations=(RELU, None), vector_gate=True)
    layer.load_state_dict(_params(d), strict=True)
    layer = layer.to(DEV).eval()
    xs = [d[k].clone().to(DEV).requires_grad_(True) for k in ("s", "v", "es", "ev")]
    so, vo = layer((xs[0], xs[1]), d["edge_index"].to(DEV), (xs[2], xs[3]))
    torch.testing.assert_close(so.detach().cpu(), d["out_s"], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(vo.detach().cpu(), d["out_v"], atol=1e-5, rtol=1e-5)
    ((so * d["g_s"].to(DEV)).sum() + (vo * d["g_v"].to(DEV)).sum()).backward()
    for t, k in zip(xs, ("grad_s", "grad_v", "grad_es", "grad_ev")):
        _scaled(t.grad, d[k], 1e-4, k)
    for k, p in layer.named_parameters():
        if p.numel():
            _scaled(p.grad, d[f"grad.{k}"], 1e-4, k)


def test_gvp_model_golden(golden):
    import gmp_amd.gvp as g
    from gmp_amd.graph import Batch
    d = golden("gvp_model.pt")
    model = g.GVPGNNModel(num_layers=2, in_dim=2, out_dim=1, s_dim=32, v_dim=4, s_dim_edge=8,
                          v_dim_edge=1)
    model.load_state_dict(_params(d), strict=True)
    model = model.to(DEV).eval()
    p = d["pos"].clone().to(DEV).requires_grad_(True)
    y = model(Batch(d["atoms"].to(DEV), p, d["edge_index"].to(DEV), d["batch"].to(DEV),
                    num_graphs=2))
    torch.testing.assert_close(y.detach().cpu(), d["out"], atol=1e-5, rtol=1e-5)
    y.sum().backward()
    _scaled(p.grad, d["grad_pos"], 1e-4, "grad_pos")


@pytest.mark.parametrize("fast,edge_linear,fused,defer", [
    (True, True, True, True), (True, True, True, False), (True, True, False, True),
    (True, False, False, True), (False, True, False, True)])
def test_gvp_conv_layer_c3_widths_vs_oracle(fast, edge_linear, fused, defer, monkeypatch):
    """defer=False: weight gradients returned through autograd after a stream join (the DDP
    configuration, dist.wrap_ddp) instead of the end-of-backward side-stream accumulation."""
    import gmp_amd.gvp as g
    from gmp_amd import ops
    monkeypatch.setattr(g, "GVP_FUSED", fused)
    monkeypatch.setattr(ops, "DEFER_WEIGHT_GRADS", defer)
    # small graphs: force the per-edge Linear path (outer-sum dW) on, or off
    monkeypatch.setattr(ops, "EDGE_LINEAR_MIN_ROWS", 1 if edge_linear else 1 << 62)
    from gmp_amd.graph import radius_graph
    torch.manual_seed(5)
    gr = radius_graph(num_nodes=600, target_edges=9000, r=2.0, seed=4, tol=0.2, shuffle=True)
    ref = ogvp.GVPConvLayer((128, 16), (32, 1), activations=(RELU, None), vector_gate=True).eval()
    with torch.no_grad():
        for prm in ref.parameters():
            if prm.dim() == 1 and prm.numel():
                prm.add_(0.1 * torch.randn_like(prm))
    lay = g.GVPConvLayer((128, 16), (32, 1), activations=(RELU, None), vector_gate=True)
    lay.load_state_dict(ref.state_dict(), strict=True)
    lay = lay.to(DEV).eval()
    if not fast:
        lay.conv._custom = True  # force the generic propagate path (reference message())
    n, e = gr.num_nodes, gr.num_edges
    s, v = torch.randn(n, 128), torch.randn(n, 16, 3)
    es, ev = torch.randn(e, 32), torch.randn(e, 1, 3)
    xs = [t.clone().to(DEV).requires_grad_(True) for t in (s, v, es, ev)]
    xr = [t.clone().requires_grad_(True) for t in (s, v, es, ev)]
    if fused:
        assert lay.conv._fast_ok((xs[0], xs[1])) and lay.conv._fused_ok((xs[0], xs[1]),
                                                                         (xs[2], xs[3]))
    so, vo = lay((xs[0], xs[1]), gr.edge_index.to(DEV), (xs[2], xs[3]))
    sr, vr = ref((xr[0], xr[1]), gr.edge_index, (xr[2], xr[3]))
    torch.testing.assert_close(so.detach().cpu(), sr.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(vo.detach().cpu(), vr.detach(), atol=1e-5, rtol=1e-5)
    gs, gv = torch.randn_like(sr), torch.randn_like(vr)
    ((so * gs.to(DEV)).sum() + (vo * gv.to(DEV)).sum()).backward()
    ((sr * gs).sum() + (vr * gv).sum()).backward()
    for a, b, nm in zip(xs, xr, ("ds", "dv", "des", "dev")):
        _scaled(a.grad, b.grad, 1e-4, nm)
    for (k, p), q in zip(lay.named_parameters(), ref.parameters()):
        if p.numel():
            _scaled(p.grad, q.grad, 1e-4, k)


@pytest.mark.parametrize("row", [0, 1])
def test_gvp_fused_out_of_range_index_raises(row):
    """An edge_index entry >= N on the fused GVPConv path raises IndexError, as the reference's
    index_select / torch_scatter do, before any receiver-sorted kernel runs (those visit only the
    in-range edges, so their per-edge outputs would hold unwritten rows)."""
    import gmp_amd.gvp as g
    from gmp_amd.graph import radius_graph
    torch.manual_seed(2)
    gr = radius_graph(num_nodes=200, target_edges=2000, r=2.0, seed=6, tol=0.2, shuffle=True)
    lay = g.GVPConvLayer((128, 16), (32, 1), activations=(RELU, None), vector_gate=True)
    lay = lay.to(DEV).eval()
    n, e = gr.num_nodes, gr.num_edges
    ei = gr.edge_index.clone()
    ei[row, e // 2] = n + 3
    x = (torch.randn(n, 128, device=DEV), torch.randn(n, 16, 3, device=DEV))
    ea = (torch.randn(e, 32, device=DEV), torch.randn(e, 1, 3, device=DEV))
    assert lay.conv._fused_ok(x, ea)
    with pytest.raises(IndexError):
        lay(x, ei.to(DEV), ea)
    so, vo = lay(x, gr.edge_index.to(DEV), ea)  # the valid graph still runs afterwards
    assert bool(torch.isfinite(so).all()) and bool(torch.isfinite(vo).all())


C3 = dict(num_layers=4, s_dim=128, v_dim=16, s_dim_edge=32, v_dim_edge=1)  # gvpgnn.py:13-27


def test_gvp_model_c3_vs_oracle():
    """Config C3 exactly (GVP-GNN 4 layers, s = 128, v = 16, edge (32, 1); gvpgnn.py:103-127)
    against the fp32 oracle and its fp64 copy (eval mode: Dropout off on both)."""
    import gmp_amd.gvp as g
    from gmp_amd.graph import Batch, radius_graph
    torch.manual_seed(6)
    gr = radius_graph(num_nodes=500, target_edges=7000, r=2.0, seed=8, tol=0.2, shuffle=True)
    ref = ogvp.GVPGNNModel(r_max=2.0, in_dim=1, out_dim=1, **C3).eval()
    model = g.GVPGNNModel(r_max=2.0, in_dim=1, out_dim=1, **C3)
    model.load_state_dict(ref.state_dict(), strict=True)
    model = model.to(DEV).eval()
    ref64 = copy.deepcopy(ref).double()
    pd = gr.pos.to(DEV).requires_grad_(True)
    y = model(Batch(gr.atoms.to(DEV), pd, gr.edge_index.to(DEV), num_graphs=1))
    pr = gr.pos.clone().requires_grad_(True)
    yr = ref(Batch(gr.atoms, pr, gr.edge_index))
    y64 = ref64(Batch(gr.atoms, gr.pos.double(), gr.edge_index))
    err = (y.detach().cpu().double() - y64.detach()).abs().max().item()
    err_ref = (yr.detach().double() - y64.detach()).abs().max().item()
    assert err <= 1e-5 * max(1.0, y64.abs().max().item()) + 2 * err_ref, (err, err_ref)
    y.sum().backward()
    yr.sum().backward()
    # d pos near r_max: the polynomial envelope's derivative is a cancellation of O(100) terms
    # in fp32 (both sides); judged against fp64 with the fp32 reference's own error as slack
    p64 = gr.pos.double().requires_grad_(True)
    ref64(Batch(gr.atoms, p64, gr.edge_index)).sum().backward()
    eg = (pd.grad.cpu().double() - p64.grad).abs().max().item()
    eg_ref = (pr.grad.double() - p64.grad).abs().max().item()
    scale = p64.grad.abs().max().item()
    assert eg <= 2e-4 * scale + 2 * eg_ref, (eg, eg_ref, scale)


@pytest.mark.parametrize("m,n,K", [(128, 144, 7777), (128, 65, 3000), (16, 128, 5000),
                                   (16, 33, 12345), (16, 16, 100), (48, 48, 0)])
def test_edge_outer_sum_rect(m, n, K):
    from gmp_amd import ops
    torch.manual_seed(m + n)
    A = torch.randn(K, m, dtype=torch.float64)
    B = torch.randn(K, n, dtype=torch.float64)
    C, cs = ops.edge_outer_sum_rect(A.float().to(DEV), B.float().to(DEV))
    ref = A.t() @ B
    assert (C.double().cpu() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    assert (cs.double().cpu() - A.sum(0)).abs().max().item() <= 1e-4
    C2, _ = ops.edge_outer_sum_rect(A.float().to(DEV), B.float().to(DEV))
    assert torch.equal(C, C2)  # deterministic


def test_gvp_fused_deterministic_and_model_c3():
    """Fused GVP message kernels: bitwise-repeatable forward/backward on a C3-width model."""
    import gmp_amd.gvp as g
    from gmp_amd.graph import Batch, radius_graph
    torch.manual_seed(11)
    gr = radius_graph(num_nodes=800, target_edges=12000, r=2.0, seed=3, tol=0.2, shuffle=True)
    model = g.GVPGNNModel(r_max=2.0, num_layers=2).to(DEV).eval()
    b = Batch(gr.atoms.to(DEV), gr.pos.to(DEV).requires_grad_(True), gr.edge_index.to(DEV))
    assert model.layers[0].conv._fused_ok((torch.zeros(1, 128, device=DEV),
                                          torch.zeros(1, 16, 3, device=DEV)),
                                         (torch.zeros(1, 32, device=DEV), None))

    def run():
        model.zero_grad()
        b.pos.grad = None
        y = model(b)
        y.sum().backward()
        return y.detach().clone(), b.pos.grad.clone(), model.layers[0].conv.message_func[1].ws.weight.grad.clone()

    a1, a2 = run(), run()
    for u, v in zip(a1, a2):
        assert torch.equal(u, v)


@pytest.mark.parametrize("E", [30000, 77, 0])
def test_gvp_edge_featurize_vs_oracle(E):
    """K1 GVP featurisation (gmp_edge_featurize_gvp_f32 + backward) against gvpgnn.py:106-112
    restated on the CPU: RadialEmbeddingBlock(|vec|) and nan_to_num(vec / |vec|); a zero-length
    edge gives a zero unit vector.  Tolerance 1e-5; d pos within 1e-5 of scale."""
    from gmp_amd import ops
    from gmp_amd.equivariant import RadialEmbeddingBlock
    from oracle.radial import RadialEmbeddingBlock as ORadial
    gen = torch.Generator().manual_seed(E + 1)
    n = max(E // 20, 4)
    pos = torch.rand(n, 3, generator=gen) * 12.0
    src = torch.randint(0, n, (E,), generator=gen)  # no self-loops: radial(0) is 0/0 upstream
    ei = torch.stack([src, (src + torch.randint(1, n, (E,), generator=gen)) % n])
    rad_p, rad_o = RadialEmbeddingBlock(10.0, 8, 5), ORadial(10.0, 8, 5)
    pd = pos.to(DEV).requires_grad_(True)
    rad, unit = ops.GvpEdgeFeaturizeFn.apply(pd, ei.to(DEV), rad_p._host)
    pr = pos.clone().requires_grad_(True)
    vec = pr[ei[0]] - pr[ei[1]]
    ln = torch.linalg.norm(vec, dim=-1, keepdim=True)
    rr, ur = rad_o(ln), torch.nan_to_num(torch.div(vec, ln))
    torch.testing.assert_close(rad.detach().cpu(), rr.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(unit.detach().cpu(), ur.detach(), atol=1e-6, rtol=1e-5)
    if E == 0:
        return
    g1, g2 = torch.randn_like(rr), torch.randn_like(ur)
    ((rad * g1.to(DEV)).sum() + (unit * g2.to(DEV)).sum()).backward()
    ((rr * g1).sum() + (ur * g2).sum()).backward()
    _scaled(pd.grad, pr.grad, 1e-5, "dpos")
    # a zero-length edge: zero unit vector
    z = torch.tensor([[1, 2], [1, 0]], device=DEV)
    _, u0 = ops.GvpEdgeFeaturizeFn.apply(pos.to(DEV), z, rad_p._host)
    assert torch.equal(u0[0].cpu(), torch.zeros(3))


def test_gvp_c3_full_size_properties():
    """C3 at full size (the 1M-edge bench graph), eval mode: forward and backward are bitwise
    deterministic, and the prediction is invariant to the input edge order and to a rotation +
    translation of the positions within 1e-5 relative (gvpgnn.py:103-127 is E(3)-invariant)."""
    import gmp_amd.gvp as g
    from gmp_amd.graph import Batch, radius_graph
    from oracle import o3 as oo3
    gr = radius_graph()  # the C2/C3 bench graph, seed 0
    torch.manual_seed(0)
    model = g.GVPGNNModel(in_dim=1, out_dim=1, **C3).to(DEV).eval()
    ei, pos, atoms = gr.edge_index.to(DEV), gr.pos.to(DEV), gr.atoms.to(DEV)

    def run(p, e, grad=True):
        model.zero_grad(set_to_none=True)
        y = model(Batch(atoms, p, e, num_graphs=1))
        if not grad:
            return y.detach().double(), None
        y.sum().backward()
        return y.detach().double(), model.layers[1].conv.message_func[1].ws.weight.grad.clone()

    with torch.no_grad():
        y0, _ = run(pos, ei, grad=False)
        yp, _ = run(pos, ei[:, torch.randperm(ei.shape[1], device=DEV)], grad=False)
        R = oo3.wigner_D(1, *(torch.tensor(a, dtype=torch.float64) for a in (0.3, 1.1, -0.6)))
        pos_r = gr.pos.double() @ R.T + torch.tensor([0.5, -2.0, 1.0], dtype=torch.float64)
        yr, _ = run(pos_r.float().to(DEV), ei, grad=False)
    scale = y0.abs().max().item()
    assert (yp - y0).abs().max().item() <= 1e-5 * scale, (yp, y0)
    assert (yr - y0).abs().max().item() <= 1e-5 * scale, (yr, y0)
    a, b = run(pos, ei), run(pos, ei)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[1].abs().max().item() > 0


@pytest.mark.parametrize("rows,C", [(50_000, 16), (1_000_003, 1), (777, 32), (5, 3), (0, 16)])
def test_vec_norm_vs_torch(rows, C):
    """GVP vector LayerNorm (gmp_vec_norm_{fwd,bwd}_f32) against the reference's torch chain
    (gvp_layer.py:232-243 with _norm_no_nan's clamp): zero channels exercise the clamp and its
    masked gradient.  Forward 1e-6 relative, gradient 1e-5 of its scale."""
    from gmp_amd.gvp import VecNormFn
    g = torch.Generator().manual_seed(rows + C)
    v = torch.randn(rows, C, 3, generator=g)
    if rows:
        v[::7, 0] = 0.0          # clamped channel
        v[1::11] *= 1e-5         # whole row near the clamp
    gout = torch.randn(rows, C, 3, generator=g)
    va = v.to(DEV).requires_grad_(True)
    y = VecNormFn.apply(va)
    (y * gout.to(DEV)).sum().backward()
    vb = v.double().requires_grad_(True)
    s2 = torch.clamp(torch.sum(torch.square(vb), -1, keepdim=True), min=1e-8)
    yr = vb / torch.sqrt(torch.mean(s2, dim=-2, keepdim=True))
    (yr * gout.double()).sum().backward()
    if rows == 0:
        assert y.shape == (0, C, 3) and va.grad.shape == (0, C, 3)
        return
    assert (y.double().cpu() - yr.detach()).abs().max().item() <= 1e-6 * max(1.0, yr.abs().max().item())
    # per row: the clamped rows' gradients are ~1e4 x the others'
    scale = vb.grad.abs().amax(dim=(1, 2))
    err = (va.grad.double().cpu() - vb.grad).abs().amax(dim=(1, 2))
    assert bool((err <= 1e-5 * scale + 1e-6).all()), (err / (scale + 1e-12)).max().item()


@pytest.mark.parametrize("rows,h", [(50_000, 32), (1_000_001, 1), (333, 33), (0, 16)])
def test_xyz_norm_vs_torch(rows, h):
    """GVP.forward's |vh| over the xyz axis (gmp_xyz_norm_{fwd,bwd}_f32) against the reference's
    _norm_no_nan(vh, axis=-2) in fp64, zero columns exercising the clamp."""
    from gmp_amd.gvp import XyzNormFn
    g = torch.Generator().manual_seed(rows + h)
    vh = torch.randn(rows, 3, h, generator=g)
    if rows:
        vh[::5, :, 0] = 0.0
    gout = torch.randn(rows, h, generator=g)
    va = vh.to(DEV).requires_grad_(True)
    y = XyzNormFn.apply(va)
    (y * gout.to(DEV)).sum().backward()
    vb = vh.double().requires_grad_(True)
    yr = torch.sqrt(torch.clamp(torch.sum(torch.square(vb), -2), min=1e-8))
    (yr * gout.double()).sum().backward()
    assert y.shape == (rows, h) and va.grad.shape == (rows, 3, h)
    if rows == 0:
        return
    assert (y.double().cpu() - yr.detach()).abs().max().item() <= 1e-6 * yr.abs().max().item()
    assert (va.grad.double().cpu() - vb.grad).abs().max().item() <= 1e-6 * vb.grad.abs().max().item() + 1e-7


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_gvp_layer_agg_backward_bitwise(reduce):
    """GvpLayerAggFn (the last message GVP with the receivers' aggregation: forward through
    gmp_gvp_layer_fwd_agg_f32, an in-wave segmented sum over the receiver-sorted edges; backward
    through gmp_gvp_layer_bwd_agg_f32, the node gradient gathered in the layer kernel's loads)
    against the unfused pair GvpLayerFn + K3 segment_reduce: forward within 1e-6 of its scale
    (the segmented scan sums a chunk in tree order, K3 sequentially), input and weight gradients
    bitwise equal (the same products in the same order).  Receivers with in-degree 0, a
    shuffled edge order."""
    import gmp_amd.gvp as g
    from gmp_amd import ops
    from gmp_amd.graph import radius_graph
    torch.manual_seed(7)
    gr = radius_graph(num_nodes=600, target_edges=9000, r=2.0, seed=4, tol=0.2, shuffle=True)
    n, E = gr.num_nodes + 5, gr.edge_index.shape[1]  # 5 receivers without edges
    recv = gr.edge_index[1].to(DEV)
    csr = ops.get_csr(recv, n)
    lay = g.GVP((128, 16), (128, 16), activations=(None, None)).to(DEV)
    W = (lay.ws.weight, lay.ws.bias, lay.wsv.weight, lay.wsv.bias, lay.wh.weight, lay.wv.weight)
    s = torch.randn(E, 128, device=DEV)
    v = torch.randn(E, 16, 3, device=DEV)
    gs = torch.randn(n, 128, device=DEV)
    gv = torch.randn(n, 16, 3, device=DEV)
    outs = []
    for fused in (True, False):
        for p in W:
            p.grad = None
        sd, vd = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
        if fused:
            a_s, a_v = g.GvpLayerAggFn.apply(sd, vd, *W, csr, reduce)
        else:
            s3, v3 = g.GvpLayerFn.apply(sd, vd, *W, False)
            a_s = ops.SegmentReduceFn.apply(s3, csr, reduce)
            a_v = ops.SegmentReduceFn.apply(v3.reshape(E, 48), csr, reduce).view(n, 16, 3)
        ((a_s * gs).sum() + (a_v * gv).sum()).backward()
        torch.cuda.synchronize()
        outs.append([a_s.detach(), a_v.detach(), sd.grad, vd.grad] + [p.grad.clone() for p in W])
    for i, (a, b) in enumerate(zip(*outs)):
        if i < 2:
            _scaled(a, b, 1e-6, f"forward {i}")
            assert a.shape == b.shape
        else:
            assert torch.equal(a, b), i
    # receivers past the last one with edges and receivers without edges: zero rows
    deg = csr.counts()
    assert bool((outs[0][0][deg == 0] == 0).all()) and bool((outs[0][1][deg == 0] == 0).all())


def test_gvp_layer_agg_no_edges():
    """The fused forward with no edges: every receiver row zero (sum and mean)."""
    import gmp_amd.gvp as g
    from gmp_amd import ops
    lay = g.GVP((128, 16), (128, 16), activations=(None, None)).to(DEV)
    W = (lay.ws.weight, lay.ws.bias, lay.wsv.weight, lay.wsv.bias, lay.wh.weight, lay.wv.weight)
    csr = ops.get_csr(torch.zeros(0, dtype=torch.int64, device=DEV), 7)
    for reduce in ("mean", "sum"):
        a_s, a_v = g.GvpLayerAggFn.apply(torch.zeros(0, 128, device=DEV),
                                         torch.zeros(0, 16, 3, device=DEV), *W, csr, reduce)
        assert a_s.shape == (7, 128) and a_v.shape == (7, 16, 3)
        assert not bool(a_s.abs().sum()) and not bool(a_v.abs().sum())


def test_gvp_msg0_bwd_agg_matches_unfused():
    """gmp_gvp_msg0_bwd_agg_f32 (receiver-sorted walk with the receiver-side sums reduced in the
    kernel) against gmp_gvp_msg0_bwd_f32 + K3: per-edge outputs bitwise equal, the receiver sums
    S_i dspre, S_i dvh, S_i dgate, S_i dvpre within 1e-6 of their scale (tree order inside a
    16-edge chunk); shuffled edges, receivers without edges."""
    from gmp_amd import _lib, ops
    from gmp_amd.graph import radius_graph
    tops = _lib.torch_ops()
    torch.manual_seed(5)
    gr = radius_graph(num_nodes=500, target_edges=8000, r=2.0, seed=6, tol=0.2, shuffle=True)
    n, E = gr.num_nodes + 3, gr.edge_index.shape[1]
    send, recv = (gr.edge_index[k].to(DEV).contiguous() for k in (0, 1))
    rcsr, scsr = ops.get_csr(recv, n), ops.get_csr(send, n)
    f = dict(device=DEV)
    P, Q = torch.randn(n, 256, **f), torch.randn(n, 288, **f)
    es, ev = torch.randn(E, 32, **f), torch.randn(E, 3, **f)
    W = [torch.randn(128, 32, **f) * 0.2, torch.randn(128, 48, **f) * 0.2, torch.randn(128, **f),
         torch.randn(16, 48, **f) * 0.2, torch.randn(16, 128, **f) * 0.1, torch.randn(16, **f),
         torch.randn(48, **f) * 0.3]
    ds, dv = torch.randn(E, 128, **f), torch.randn(E, 48, **f)
    ref = tops.gvp_msg0_bwd(send, recv, P, Q, es, ev, W, ds, dv, False)
    got = tops.gvp_msg0_bwd_agg(send, recv, P, Q, es, ev, W, ds, dv, rcsr.perm, rcsr.rowptr, n,
                                False)
    torch.cuda.synchronize()
    for k in (0, 2, 3, 5, 6, 7, 8):
        assert torch.equal(got[k], ref[k]), k
    for k, src in ((9, ref[0]), (10, ref[6]), (11, ref[2]), (12, ref[5])):
        want, _ = ops.segment_reduce(src, rcsr, "sum")
        _scaled(got[k], want, 1e-6, f"receiver sum {k}")
    assert bool((got[9][rcsr.counts() == 0] == 0).all())


@pytest.mark.parametrize("E,so", [(200_000, 32), (1000, 16), (5, 32), (0, 32)])
def test_gvp_edge_embed_vs_oracle(E, so):
    """K1e (gmp_gvp_edge_embed_{fwd,bwd}_f32): W_e = LayerNorm((8, 1)) + GVP((8, 1), (so, 1))
    (gvpgnn.py:73-77) against the oracle modules in fp64 on the same parameters (random LayerNorm
    affine, a negative wh, some zero-length unit rows): es / ev within 1e-5, every parameter
    gradient within 3e-5 of its scale (fp32 sums over up to 200k edge rows, some with
    cancellation: the LayerNorm gradients are sums over the 32 output channels); bitwise
    repeatable."""
    import gmp_amd.gvp as g
    torch.manual_seed(E + so)
    ref = torch.nn.Sequential(ogvp.LayerNorm((8, 1)),
                              ogvp.GVP((8, 1), (so, 1), activations=(None, None),
                                       vector_gate=True))
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
        ref[1].wh.weight.fill_(-0.8)
    mod = torch.nn.Sequential(g.LayerNorm((8, 1)),
                              g.GVP((8, 1), (so, 1), activations=(None, None), vector_gate=True))
    mod.load_state_dict(ref.state_dict(), strict=True)
    mod = mod.to(DEV)
    rad = torch.rand(E, 8) * 2
    unit = torch.nn.functional.normalize(torch.randn(E, 3), dim=-1)
    unit[::97] = 0.0                                      # zero-length edges
    des, dev = torch.randn(E, so), torch.randn(E, 1, 3)
    assert g._edge_embed_ok(mod, rad.to(DEV), unit.to(DEV))

    def fused():
        mod.zero_grad(set_to_none=True)
        es, ev = g.edge_embed(mod, rad.to(DEV), unit.to(DEV))
        ((es * des.to(DEV)).sum() + (ev * dev.to(DEV)).sum()).backward()
        return es, ev, {k: p.grad.clone() for k, p in mod.named_parameters() if p.numel()}

    es, ev, gr = fused()
    ref64 = copy.deepcopy(ref).double()
    es_r, ev_r = ref64((rad.double(), unit.double().unsqueeze(-2)))
    ((es_r * des.double()).sum() + (ev_r * dev.double()).sum()).backward()
    assert es.shape == (E, so) and ev.shape == (E, 1, 3)
    if E:
        torch.testing.assert_close(es.cpu().double(), es_r.detach(), atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(ev.cpu().double(), ev_r.detach(), atol=1e-5, rtol=1e-5)
    for k, p in ref64.named_parameters():
        if p.numel():
            _scaled(gr[k].double(), p.grad, 3e-5, k)
    es2, ev2, gr2 = fused()
    assert torch.equal(es, es2) and torch.equal(ev, ev2)
    assert all(torch.equal(gr[k], gr2[k]) for k in gr)


def test_gvp_model_c3_edge_embed_fused_vs_chain():
    """The C3 model with positions without requires_grad (the bench step) takes K1e; against the
    fp64 oracle model its output and every parameter gradient are no worse than 1e-5 / 1e-4 of
    scale + 2x those of the module-chain edge embedding (EDGE_EMBED_FUSED = False).  (The two
    embeddings differ in the last bits of es / ev; through four layers a feed-forward ReLU input
    sitting within rounding of 0 can take the other branch in one of them and move a weight sum
    by ~1e-4 of scale, so fp64 is the yardstick rather than a direct 1e-4 comparison.)"""
    import gmp_amd.gvp as g
    from gmp_amd.graph import Batch, radius_graph
    torch.manual_seed(12)
    gr = radius_graph(num_nodes=600, target_edges=9000, r=2.0, seed=5, tol=0.2, shuffle=True)
    ref = ogvp.GVPGNNModel(r_max=2.0, in_dim=1, out_dim=1, **C3).eval()
    model = g.GVPGNNModel(r_max=2.0, in_dim=1, out_dim=1, **C3)
    model.load_state_dict(ref.state_dict(), strict=True)
    model = model.to(DEV).eval()
    b = Batch(gr.atoms.to(DEV), gr.pos.to(DEV), gr.edge_index.to(DEV))

    def run(fused):
        g.EDGE_EMBED_FUSED = fused
        try:
            model.zero_grad(set_to_none=True)
            y = model(b)
            y.sum().backward()
        finally:
            g.EDGE_EMBED_FUSED = True
        return y.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()
                                    if p.grad is not None}

    y1, g1 = run(True)
    y0, g0 = run(False)
    assert set(g1) == set(g0)
    ref64 = copy.deepcopy(ref).double()
    p1 = []  # the feed-forward ReLU inputs (first FF GVP's scalar Linear) of every layer
    hooks = [lay.ff_func[0].ws.register_forward_hook(lambda m, i, o: p1.append(o.detach().abs()))
             for lay in ref64.layers]
    y64 = ref64(Batch(gr.atoms, gr.pos.double(), gr.edge_index))
    for h in hooks:
        h.remove()
    y64.sum().backward()
    r64 = {k: p.grad for k, p in ref64.named_parameters() if p.grad is not None}
    e1 = (y1.cpu().double() - y64.detach()).abs().max().item()
    e0 = (y0.cpu().double() - y64.detach()).abs().max().item()
    assert e1 <= 1e-5 * max(1.0, y64.abs().max().item()) + 2 * e0, (e1, e0)
    # a ReLU input within fp32 rounding of 0 (1e-6 of the layer's largest) can take either branch
    # in a correct fp32 evaluation; where one exists the gradient bound is 1e-3 of scale
    kink = min((t.min() / t.max()).item() for t in p1)
    tol = 1e-3 if kink < 1e-6 else 1e-4
    for k in g0:
        t = r64[k]
        e1 = (g1[k].cpu().double() - t).abs().max().item()
        e0 = (g0[k].cpu().double() - t).abs().max().item()
        assert e1 <= tol * t.abs().max().item() + 2 * e0 + 1e-6, (k, e1, e0, kink)


@pytest.mark.parametrize("K,C", [(999_722, 48), (999_722, 16), (1000, 48), (77, 16), (0, 48)])
def test_edge_xyz_dot(K, C):
    """gmp_edge_xyz_dot_f32: out[c] = sum_(e,x) A[e, 3c + x] v[e, x] against fp64 torch, within
    1e-5 of scale; bitwise repeatable (fixed-order partial rows)."""
    from gmp_amd import _lib
    torch.manual_seed(K + C)
    A = torch.randn(K, 3 * C)
    v = torch.randn(K, 3)
    xdot = _lib.torch_ops().edge_xyz_dot
    out = xdot(A.to(DEV), v.to(DEV))
    ref = (A.double().view(K, C, 3) * v.double().view(K, 1, 3)).sum((0, 2))
    assert out.shape == (C,)
    _scaled(out.double(), ref, 1e-5, "xyz_dot")
    assert torch.equal(out, xdot(A.to(DEV), v.to(DEV)))


def _ff_pair(seed):
    """GVPConvLayer's node feed-forward (gvp_layer.py:361-366) as oracle modules, biases and
    weights perturbed away from the init."""
    torch.manual_seed(seed)
    ff = torch.nn.Sequential(ogvp.GVP((128, 16), (512, 32), activations=(RELU, None),
                                      vector_gate=True),
                             ogvp.GVP((512, 32), (128, 16), activations=(None, None),
                                      vector_gate=True))
    with torch.no_grad():
        for p in ff.parameters():
            if p.numel():
                p.add_(0.05 * torch.randn_like(p))
    return ff


def _ff_inputs(n, seed):
    torch.manual_seed(seed)
    s, v = torch.randn(n, 128), torch.randn(n, 16, 3)
    if n > 8:
        v[3] = 0.0           # every |vh| of both GVPs at the clamp (zero gradient there)
        v[5, :8] = 0.0
    return s, v


@pytest.mark.parametrize("n", [1, 13, 1000, 4099])
def test_gvp_ff_fused_vs_oracle(n):
    """K17 (gmp_gvp_ff_{fwd,bwd}_f32) against the oracle's two GVPs in fp64: outputs at 1e-5 of
    scale, input and weight gradients at 1e-4 of scale (and no worse than 2x the fp32 oracle);
    ragged node counts, zero vectors (clamped norms)."""
    import gmp_amd.gvp as g
    ref = _ff_pair(31 + n)
    ref64 = copy.deepcopy(ref).double()
    lay = torch.nn.Sequential(g.GVP((128, 16), (512, 32), activations=(RELU, None),
                                    vector_gate=True),
                              g.GVP((512, 32), (128, 16), activations=(None, None),
                                    vector_gate=True))
    lay.load_state_dict(ref.state_dict())
    lay = lay.to(DEV)
    s, v = _ff_inputs(n, n)
    sd, vd = s.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    assert g._ff_fusable(lay, (sd, vd))
    so, vo = g.gvp_ff(lay, (sd, vd))
    s64, v64 = s.double().requires_grad_(True), v.double().requires_grad_(True)
    sr, vr = ref64((s64, v64))
    s32, v32 = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
    sr32, vr32 = ref((s32, v32))
    for a, b, b32, nm in ((so, sr, sr32, "s"), (vo, vr, vr32, "v")):
        err = (a.detach().cpu().double() - b.detach()).abs().max().item()
        e32 = (b32.detach().double() - b.detach()).abs().max().item()
        assert err <= 1e-5 * max(1.0, b.abs().max().item()) + 2 * e32, (nm, err, e32)
    torch.manual_seed(7)
    gs, gv = torch.randn(n, 128), torch.randn(n, 16, 3)
    ((so * gs.to(DEV)).sum() + (vo * gv.to(DEV)).sum()).backward()
    ((sr * gs.double()).sum() + (vr * gv.double()).sum()).backward()
    ((sr32 * gs).sum() + (vr32 * gv).sum()).backward()
    pairs = [("ds", sd.grad, s64.grad, s32.grad), ("dv", vd.grad, v64.grad, v32.grad)]
    pairs += [(k, p.grad, q.grad, r.grad) for (k, p), q, r in
              zip(lay.named_parameters(), ref64.parameters(), ref.parameters()) if p.numel()]
    for nm, a, b, b32 in pairs:
        err = (a.cpu().double() - b).abs().max().item()
        e32 = (b32.double() - b).abs().max().item()
        sc = b.abs().max().item()
        assert err <= 1e-4 * sc + 2 * e32 + 1e-7, f"{nm}: {err:.3e} (fp32 oracle {e32:.3e}, " \
                                                  f"scale {sc:.3e})"


def test_gvp_ff_fused_matches_chain_and_is_deterministic():
    """At the C3 node count (50k): two runs of K17 bitwise equal, and K17 against the fp64 oracle
    no worse than 1e-5 (outputs) / 1e-4 (gradients) of scale + 2x the module chain's own error
    on the device.  (At 50k rows some first-GVP pre-activations sit within fp32 rounding of the
    ReLU kink -- row 16341 here at 3.6e-8 -- and a correct fp32 evaluation may take the other
    branch there: the reference's torch ops on the device do, scripts/dbg_gvp_chain.py; that row
    moves the weight sums by ~1e-4 of scale, so fp64 is the yardstick, as elsewhere.)"""
    import gmp_amd.gvp as g
    ref = _ff_pair(5)
    lay = torch.nn.Sequential(g.GVP((128, 16), (512, 32), activations=(RELU, None),
                                    vector_gate=True),
                              g.GVP((512, 32), (128, 16), activations=(None, None),
                                    vector_gate=True))
    lay.load_state_dict(ref.state_dict())
    lay = lay.to(DEV)
    n = 50_000
    s, v = _ff_inputs(n, 3)
    torch.manual_seed(9)
    gs, gv = torch.randn(n, 128), torch.randn(n, 16, 3)

    def run(fused):
        g.GVP_FF_FUSED = fused
        try:
            lay.zero_grad(set_to_none=True)
            sd, vd = s.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
            so, vo = g.gvp_ff(lay, (sd, vd))
            ((so * gs.to(DEV)).sum() + (vo * gv.to(DEV)).sum()).backward()
            return [so.detach(), vo.detach(), sd.grad, vd.grad] + \
                [p.grad.clone() for p in lay.parameters() if p.numel()]
        finally:
            g.GVP_FF_FUSED = True

    a, b, c = run(True), run(True), run(False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ref64 = copy.deepcopy(ref).double()
    s64, v64 = s.double().requires_grad_(True), v.double().requires_grad_(True)
    so, vo = ref64((s64, v64))
    ((so * gs.double()).sum() + (vo * gv.double()).sum()).backward()
    r = [so.detach(), vo.detach(), s64.grad, v64.grad] + \
        [p.grad for p in ref64.parameters() if p.numel()]
    for i, (x, y, t) in enumerate(zip(a, c, r)):
        ef = (x.cpu().double() - t).abs().max().item()
        ec = (y.cpu().double() - t).abs().max().item()
        sc = t.abs().max().item()
        tol = (1e-5 * max(sc, 1.0)) if i < 2 else 1e-4 * sc
        assert ef <= tol + 2 * ec + 1e-7, (i, ef, ec, sc)


def test_gvp_model_c3_uses_fused_ff():
    """The C3 model runs K17 in every layer (no module-chain fallback)."""
    import gmp_amd.gvp as g
    from gmp_amd.graph import radius_graph, Batch
    model = g.GVPGNNModel(r_max=2.0, **C3).to(DEV).eval()
    gr = radius_graph(num_nodes=300, target_edges=3000, r=2.0, seed=2, tol=0.3)
    calls = []
    orig = g.GvpFFFn.apply

    def spy(*a):
        calls.append(1)
        return orig(*a)
    g.GvpFFFn.apply = spy
    try:
        model(Batch(gr.atoms.to(DEV), gr.pos.to(DEV), gr.edge_index.to(DEV)))
    finally:
        g.GvpFFFn.apply = orig
    assert len(calls) == C3["num_layers"]


@pytest.mark.parametrize("n", [0, 262_143, 262_144])
def test_gvp_ff_fused_at_weight_sum_thresholds(n):
    """K17 forward + backward where its four weight sums (576 x 192, 192 x 576, 192 x 64,
    192 x 128 over the nodes) change route: no nodes (zero fill / library GEMM), the last
    node-level size (quadrant kernel) and the first split-plane size (192 x 64 only; the other
    three go to the library GEMM).  Reference: the oracle's two GVPs in fp64 on the device;
    bounds as test_gvp_ff_fused_vs_oracle (1e-5 of scale for outputs, 1e-4 of scale for
    gradients, plus twice the error of the oracle's fp32 chain on the device).  n = 0: outputs
    with no rows and exact zeros for all twelve parameter gradients."""
    import gmp_amd.gvp as g
    ref = _ff_pair(77)
    ref64 = copy.deepcopy(ref).double().to(DEV)
    ref32 = copy.deepcopy(ref).to(DEV)
    lay = torch.nn.Sequential(g.GVP((128, 16), (512, 32), activations=(RELU, None),
                                    vector_gate=True),
                              g.GVP((512, 32), (128, 16), activations=(None, None),
                                    vector_gate=True))
    lay.load_state_dict(ref.state_dict())
    lay = lay.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(n + 3)
    s = torch.randn(n, 128, generator=gen, device=DEV)
    v = torch.randn(n, 16, 3, generator=gen, device=DEV)
    gs = torch.randn(n, 128, generator=gen, device=DEV)
    gv = torch.randn(n, 16, 3, generator=gen, device=DEV)
    if n:
        v[3] = 0.0           # every |vh| of both GVPs at the clamp
        v[5, :8] = 0.0
        # Of n x 512 first-GVP pre-activations some thousand lie within fp32 rounding of the ReLU
        # kink, where a correct fp32 evaluation may take the other branch than fp64 (as in
        # test_gvp_ff_fused_matches_chain_and_is_deterministic); each such row moves the
        # gradients by more than the bounds and would hide a lost row behind the fp32 chain's
        # allowance.  Rows with a pre-activation within 1e-4 of zero (fp32 rounding there:
        # ~1e-6) get new scalars until none is left, so the bounds below are about arithmetic.
        g1 = ref64[0]
        with torch.no_grad():
            vn = ogvp.norm_no_nan(g1.wh(v.double().transpose(-1, -2)), axis=-2)
        for _ in range(8):
            with torch.no_grad():
                pre = g1.ws(torch.cat([s.double(), vn], -1))
            near = (pre.abs() < 1e-4).any(1)
            if not near.any():
                break
            s[near] = torch.randn(int(near.sum()), 128, generator=gen, device=DEV)
        assert not near.any()

    def run(f, dt):
        si, vi = s.to(dt).clone().requires_grad_(True), v.to(dt).clone().requires_grad_(True)
        so, vo = f((si, vi))
        ((so * gs.to(dt)).sum() + (vo * gv.to(dt)).sum()).backward()
        return so.detach(), vo.detach(), si.grad, vi.grad

    assert g._ff_fusable(lay, (s, v))
    got = run(lambda x: g.gvp_ff(lay, x), torch.float32)
    torch.cuda.synchronize()
    want, w32 = run(ref64, torch.float64), run(ref32, torch.float32)
    named = [(k, p) for k, p in lay.named_parameters() if p.numel()]
    assert len(named) == 12 and all(p.grad is not None for _, p in named)
    if n == 0:
        assert got[0].shape == (0, 128) and got[1].shape == (0, 16, 3)
        assert got[2].shape == (0, 128) and got[3].shape == (0, 16, 3)
        for k, p in named:
            assert torch.count_nonzero(p.grad).item() == 0, k
        return
    for i, nm in enumerate(("s", "v")):
        err = (got[i].double() - want[i]).abs().max().item()
        e32 = (w32[i].double() - want[i]).abs().max().item()
        assert err <= 1e-5 * max(1.0, want[i].abs().max().item()) + 2 * e32, (nm, err, e32)
    pairs = [("ds", got[2], want[2], w32[2]), ("dv", got[3], want[3], w32[3])]
    pairs += [(k, p.grad, q.grad, r.grad) for (k, p), q, r in
              zip(named, [q for q in ref64.parameters() if q.numel()],
                  [r for r in ref32.parameters() if r.numel()])]
    for nm, a, b, b32 in pairs:
        err = (a.double() - b).abs().max().item()
        e32 = (b32.double() - b).abs().max().item()
        sc = b.abs().max().item()
        print(f"n={n} {nm}: err {err:.3e} fp32 chain {e32:.3e} scale {sc:.3e}")
        assert err <= 1e-4 * sc + 2 * e32 + 1e-7, f"{nm}: {err:.3e} (fp32 chain {e32:.3e}, " \
                                                  f"scale {sc:.3e})"


def test_gvp_conv_layer_empty_node_mask(monkeypatch):
    """GVPConvLayer forward + backward with a node_mask that selects nothing: the feed-forward
    sees no rows (K17's weight sums at K = 0).  With GVP_FF_FUSED on and off the outputs and
    every gradient are identical, and they are the CPU oracle's for the same mask: the inputs
    returned unchanged, the output gradient passed through, zeros for every parameter."""
    import gmp_amd.gvp as g
    from gmp_amd.graph import radius_graph
    torch.manual_seed(8)
    gr = radius_graph(num_nodes=200, target_edges=2000, r=2.0, seed=6, tol=0.2, shuffle=True)
    ref = ogvp.GVPConvLayer((128, 16), (32, 1), activations=(RELU, None), vector_gate=True).eval()
    n, e = gr.num_nodes, gr.num_edges
    s, v = torch.randn(n, 128), torch.randn(n, 16, 3)
    es, ev = torch.randn(e, 32), torch.randn(e, 1, 3)
    gs, gv = torch.randn(n, 128), torch.randn(n, 16, 3)
    mask = torch.zeros(n, dtype=torch.bool)

    def run(layer, dev):
        layer.zero_grad(set_to_none=True)
        leaves = [t.clone().to(dev).requires_grad_(True) for t in (s, v, es, ev)]
        # the layer writes the selected rows into its input in place: not into a leaf
        so, vo = layer((leaves[0].clone(), leaves[1].clone()), gr.edge_index.to(dev),
                       (leaves[2], leaves[3]), node_mask=mask.to(dev))
        ((so * gs.to(dev)).sum() + (vo * gv.to(dev)).sum()).backward()
        if dev != "cpu":
            torch.cuda.synchronize()
        out = {"so": so.detach(), "vo": vo.detach()}
        out.update({f"d{i}": t.grad for i, t in enumerate(leaves)})
        out.update({k: p.grad for k, p in layer.named_parameters() if p.numel()})
        return {k: (None if t is None else t.detach().cpu().clone()) for k, t in out.items()}

    want = run(ref, "cpu")
    assert torch.equal(want["so"], s) and torch.equal(want["d0"], gs)
    lay = g.GVPConvLayer((128, 16), (32, 1), activations=(RELU, None), vector_gate=True)
    lay.load_state_dict(ref.state_dict(), strict=True)
    lay = lay.to(DEV).eval()
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(g, "GVP_FF_FUSED", fused)
        res[fused] = run(lay, DEV)
    assert set(res[True]) == set(res[False]) == set(want)
    for k, w in want.items():
        a, b = res[True][k], res[False][k]
        assert (a is None) == (b is None) == (w is None), k
        if w is not None:
            assert torch.equal(a, b), k
            assert torch.equal(a, w), k
