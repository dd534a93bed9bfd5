"""K4 without the work nobody reads (ops.EGNN_SKIP_DEAD_POS): the mlp_pos branch of a layer whose
position output is unused, and the position gradient when pos does not require grad.  The
variants only leave work out, so everything a caller sees is compared bitwise (torch.equal)
against the full kernels (the switch off)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _edges(n, seed):
    """~3.3k edges on n = 300 nodes: receivers 280.. have no in-edge, node 9 has 40, node 5 has
    200 (carries across 16-edge chunks and across a wave's chunk range), E is no multiple of 16,
    edges shuffled."""
    gen = torch.Generator().manual_seed(seed)
    recv = torch.randint(0, 280, (3000,), generator=gen)
    send = torch.randint(0, n, (3000,), generator=gen)
    keep = recv != send
    recv, send = recv[keep], send[keep]
    hub = torch.randperm(n - 1, generator=gen)
    s5 = hub[:200] + (hub[:200] >= 5).long()   # 200 distinct senders != 5
    s9 = hub[200:240] + (hub[200:240] >= 9).long()
    recv = torch.cat([recv, torch.full((200,), 5), torch.full((40,), 9)])
    send = torch.cat([send, s5, s9])
    if recv.numel() % 16 == 0:
        recv, send = torch.cat([recv, torch.tensor([7])]), torch.cat([send, torch.tensor([8])])
    perm = torch.randperm(recv.numel(), generator=gen)
    ei = torch.stack([send[perm], recv[perm]])
    deg = torch.bincount(ei[1], minlength=n)
    assert ei.shape[1] % 16 and (deg == 0).any() and deg[9] > 16 and deg[5] > 128
    pos = torch.randn(n, 3, generator=gen) * 2.0
    return ei, pos


def _layer(d, act, aggr, seed):
    import gmp_amd
    torch.manual_seed(seed)
    lay = gmp_amd.EGNNLayer(d, act, "layer", aggr).to(DEV)
    with torch.no_grad():
        for p in lay.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return lay


def _run_layer(lay, h, pos, ei, gh, pos_grad, monkeypatch, skip):
    """Loss on ho alone; (ho, dh, dpos or None, {name: grad})."""
    from gmp_amd import ops
    monkeypatch.setattr(ops, "EGNN_SKIP_DEAD_POS", skip)
    lay.zero_grad(set_to_none=True)
    hd = h.clone().requires_grad_(True)
    pd = pos.clone().requires_grad_(pos_grad)
    ho, _ = lay(hd, pd, ei)
    (ho * gh).sum().backward()
    torch.cuda.synchronize()
    return ho.detach(), hd.grad, pd.grad, {k: p.grad for k, p in lay.named_parameters()}


def _compare_layer(lay, h, pos, ei, monkeypatch):
    gh = torch.randn(h.shape, device=DEV)
    for pos_grad in (True, False):
        off = _run_layer(lay, h, pos, ei, gh, pos_grad, monkeypatch, False)
        on = _run_layer(lay, h, pos, ei, gh, pos_grad, monkeypatch, True)
        assert torch.equal(off[0], on[0]), "ho"
        assert torch.equal(off[1], on[1]), "dh"
        if pos_grad:
            assert torch.equal(off[2], on[2]), "dpos"
        else:
            assert on[2] is None
        for k in off[3]:
            assert off[3][k] is not None and on[3][k] is not None, k
            assert torch.equal(off[3][k], on[3][k]), (k, pos_grad)
            if k.startswith("mlp_pos"):
                assert on[3][k].abs().max().item() == 0.0, k
    return off


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("act", ["relu", "swish"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_layer_bitwise(d, act, aggr, f32, monkeypatch):
    """One layer, loss on ho only: ho, dh, dpos and every parameter gradient identical with the
    optimisation on and off; mlp_pos gradients are zero tensors (present) in both; the same with
    pos.requires_grad = False (then no dpos)."""
    from gmp_amd import _lib
    lib = _lib.load()
    ei, pos = _edges(300, seed=d)
    lay = _layer(d, act, aggr, seed=d + 1)
    h = torch.randn(300, d, device=DEV)
    prev = lib.gmp_egnn_set_f32_mfma(int(f32))
    try:
        off = _compare_layer(lay, h, pos.to(DEV), ei.to(DEV), monkeypatch)
    finally:
        lib.gmp_egnn_set_f32_mfma(prev)
    assert off[1].abs().max().item() > 0 and off[3]["mlp_msg.3.weight"].abs().max().item() > 0


@pytest.mark.parametrize("n,e", [(1, 0), (5, 0)])
def test_layer_no_edges(n, e, monkeypatch):
    lay = _layer(64, "relu", "sum", seed=3)
    h = torch.randn(n, 64, device=DEV)
    pos = torch.randn(n, 3, device=DEV)
    ei = torch.zeros((2, e), dtype=torch.long, device=DEV)
    _compare_layer(lay, h, pos, ei, monkeypatch)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _raw_params(d, seed):
    torch.manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV)
    return [r(d), 0.1 * r(d), 1 + 0.1 * r(d), 0.1 * r(d), r(d, d) / d ** 0.5, 0.1 * r(d),
            1 + 0.1 * r(d), 0.1 * r(d), r(d, d) / d ** 0.5, 0.1 * r(d), 1 + 0.1 * r(d), 0.1 * r(d),
            r(d), r(1)]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("d,act,mean", [(32, 1, True), (64, 0, False), (128, 0, True),
                                        (128, 1, False)])
def test_forward_op_without_pos_branch(d, act, mean, f32):
    """torch.ops.gmp.egnn_edge_fwd(need_pos=False): m_aggr, x_hat1, x_hat2 and rstd[:, :2] are the
    full forward's, pos_aggr has no rows; inference form too."""
    from gmp_amd import _lib, ops
    lib = _lib.load()
    ei, pos = _edges(300, seed=11)
    graph = ops.egnn_graph(ei.to(DEV), 300)
    params = _raw_params(d, seed=d)
    AB = torch.randn(300, 2 * d, device=DEV)
    args = (AB, pos.to(DEV), graph.rowptr, graph.recv, graph.send, params, act, mean, 1e-5)
    tops = _lib.torch_ops()
    prev = lib.gmp_egnn_set_f32_mfma(int(f32))
    try:
        m0, p0, xh0, rs0 = tops.egnn_edge_fwd(*args, True, 2)
        m1, p1, xh1, rs1 = tops.egnn_edge_fwd(*args, True, 2, False)
        m2, p2, xh2, rs2 = tops.egnn_edge_fwd(*args, False, 2, False)
    finally:
        lib.gmp_egnn_set_f32_mfma(prev)
    assert tuple(p0.shape) == (300, 3) and tuple(p1.shape) == (0, 3) and tuple(p2.shape) == (0, 3)
    assert torch.equal(m0, m1) and torch.equal(m0, m2)
    assert torch.equal(xh0, xh1) and torch.equal(rs0[:, :2], rs1[:, :2])
    assert xh2.shape[0] == 0 and rs2.shape[0] == 0
    assert m0.abs().max().item() > 0


def _model_run(model, b, monkeypatch, skip, pos_grad=False):
    from gmp_amd import ops
    monkeypatch.setattr(ops, "EGNN_SKIP_DEAD_POS", skip)
    model.zero_grad(set_to_none=True)
    b.pos = b.pos.detach().clone().requires_grad_(pos_grad)
    out = model(b)
    out.sum().backward()
    torch.cuda.synchronize()
    return out.detach(), b.pos.grad, {k: p.grad for k, p in model.named_parameters()}


@pytest.fixture(scope="module")
def model_graph():
    from gmp_amd.graph import radius_graph
    return radius_graph(num_nodes=3000, target_edges=60_000, r=2.0, seed=5, tol=0.2,
                        shuffle=True).to(DEV)


@pytest.mark.parametrize("pos_grad", [False, True])
def test_model_bitwise(model_graph, pos_grad, monkeypatch):
    """EGNNModel(3 x 128): prediction, every parameter gradient (and dpos, force-style) identical
    on / off; the last layer's mlp_pos gradients are zero tensors."""
    import gmp_amd
    torch.manual_seed(0)
    model = gmp_amd.EGNNModel(num_layers=3, emb_dim=128, in_dim=1, out_dim=1).to(DEV)
    off = _model_run(model, model_graph, monkeypatch, False, pos_grad)
    on = _model_run(model, model_graph, monkeypatch, True, pos_grad)
    assert torch.equal(off[0], on[0])
    if pos_grad:
        assert torch.equal(off[1], on[1]) and on[1].abs().max().item() > 0
    for k in off[2]:
        assert off[2][k] is not None and on[2][k] is not None, k
        assert torch.equal(off[2][k], on[2][k]), k
        if k.startswith("convs.2.mlp_pos"):
            assert on[2][k].abs().max().item() == 0.0, k
    assert on[2]["convs.1.mlp_pos.0.weight"].abs().max().item() > 0


def _count_launches(monkeypatch):
    """Records (kind, ...) for every K4 launch, dW3-style outer sum and (E, 3) segment sum."""
    from gmp_amd import _lib, ops
    log = []
    tops = _lib.torch_ops()

    class Tops:
        def __getattr__(self, name):
            fn = getattr(tops, name)
            if name == "egnn_edge_fwd":
                return lambda *a: log.append(("fwd", a[11] if len(a) > 11 else True)) or fn(*a)
            if name == "egnn_edge_bwd":
                return lambda *a: log.append(("bwd", a[12] if len(a) > 12 else True,
                                              a[13] if len(a) > 13 else True)) or fn(*a)
            return fn

    proxy = Tops()
    monkeypatch.setattr(_lib, "torch_ops", lambda: proxy)
    outer, seg = ops.edge_outer_sum_act, ops.segment_reduce
    monkeypatch.setattr(ops, "edge_outer_sum_act",
                        lambda *a, **k: log.append(("outer",)) or outer(*a, **k))
    monkeypatch.setattr(ops, "segment_reduce",
                        lambda src, *a, **k: log.append(("seg", src.shape[1])) or seg(src, *a, **k))
    return log


def test_model_skips_dead_launches(model_graph, monkeypatch):
    """Default model (3 layers): the last layer runs the forward and backward without the
    position branch and launches no dW3 sum; layer 0 launches no gdiff reduction.  With
    equivariant_pred every layer takes the full forward and the full position branch."""
    import gmp_amd
    torch.manual_seed(0)
    model = gmp_amd.EGNNModel(num_layers=3, emb_dim=128, in_dim=1, out_dim=1).to(DEV)
    ref = _model_run(model, model_graph, monkeypatch, True)
    log = _count_launches(monkeypatch)
    got = _model_run(model, model_graph, monkeypatch, True)
    assert torch.equal(ref[0], got[0])
    assert [x[1] for x in log if x[0] == "fwd"] == [True, True, False]
    # backward order: layer 2, 1, 0 -> (pos_branch, pos_grad)
    assert [x[1:] for x in log if x[0] == "bwd"] == [(False, True), (True, True), (True, False)]
    assert sum(x[0] == "outer" for x in log) == 5       # dW2 x 3, dW3 x 2
    assert sum(x == ("seg", 3) for x in log) == 2       # gdiff sums of layers 2 and 1 only

    log.clear()
    torch.manual_seed(0)
    eq = gmp_amd.EGNNModel(num_layers=3, emb_dim=128, in_dim=1, out_dim=1,
                           equivariant_pred=True).to(DEV)
    on = _model_run(eq, model_graph, monkeypatch, True)
    assert [x[1] for x in log if x[0] == "fwd"] == [True, True, True]
    assert [x[1] for x in log if x[0] == "bwd"] == [True, True, True]
    assert sum(x[0] == "outer" for x in log) == 6
    off = _model_run(eq, model_graph, monkeypatch, False)
    assert torch.equal(on[0], off[0])
    for k in on[2]:
        assert torch.equal(on[2][k], off[2][k]), k
    assert on[2]["convs.2.mlp_pos.0.weight"].abs().max().item() > 0


def test_ex_entry_points_null_pointers():
    """gmp_egnn_edge_{fwd,bwd}_ex_f32: a null required pointer is GMP_ERR_ARG; the outputs (and
    g_pos_aggr) that a variant skips may be null; unknown flag bits are refused."""
    from gmp_amd import _lib, ops
    lib = _lib.load()
    d, n = 32, 300
    ei, pos = _edges(n, seed=2)
    graph = ops.egnn_graph(ei.to(DEV), n)
    E = ei.shape[1]
    pos = pos.to(DEV)
    params = _raw_params(d, seed=1)
    P = _lib.GmpEgnnParams(*[t.data_ptr() for t in params])
    f = dict(device=DEV)
    AB = torch.randn(n, 2 * d, **f)
    m, pa = torch.empty(n, d, **f), torch.empty(n, 3, **f)
    xh, rs = torch.empty(2, E, d, **f), torch.empty(E, 3, **f)
    NB, NG = _lib.EGNN_NO_POS_BRANCH, _lib.EGNN_NO_POS_GRAD
    s = torch.cuda.current_stream().cuda_stream

    def fwd(flags, m_=m, pa_=pa):
        return lib.gmp_egnn_edge_fwd_ex_f32(
            n, E, d, AB.data_ptr(), pos.data_ptr(), graph.rowptr.data_ptr(),
            graph.recv.data_ptr(), graph.send.data_ptr(), ctypes.byref(P), 0, 0, 1e-5,
            _ptr(m_), _ptr(pa_), xh.data_ptr(), 2, rs.data_ptr(), flags, s)

    assert fwd(0) == 0
    assert fwd(0, pa_=None) == _lib.GMP_ERR_ARG
    assert fwd(NB, m_=None) == _lib.GMP_ERR_ARG
    assert fwd(NG) == _lib.GMP_ERR_ARG and fwd(4) == _lib.GMP_ERR_ARG
    m_full = m.clone()
    assert fwd(NB, pa_=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(m, m_full)

    gm, gp = torch.randn(n, d, **f), torch.zeros(n, 3, **f)
    rows = lib.gmp_egnn_edge_bwd_partials_rows(E, d)
    out = dict(dA=torch.empty(n, d, **f), dpr=torch.empty(n, 3, **f), dp1=torch.empty(E, d, **f),
               gd=torch.empty(E, 3, **f), dp2=torch.empty(E, d, **f), dp3=torch.empty(E, d, **f),
               part=torch.empty(rows, 8 * d + 1, **f))
    amax = torch.zeros(2, dtype=torch.int32, **f)

    def bwd(flags, gp_=gp, amax_=amax, **null):
        o = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
        return lib.gmp_egnn_edge_bwd_ex_f32(
            n, E, d, pos.data_ptr(), graph.rowptr.data_ptr(), graph.recv.data_ptr(),
            graph.send.data_ptr(), ctypes.byref(P), 0, 0, xh.data_ptr(), 2, rs.data_ptr(),
            gm.data_ptr(), _ptr(gp_), o["dA"], o["dpr"], o["dp1"], o["gd"], o["dp2"],
            o["dp3"], o["part"], _ptr(amax_), flags, s)

    assert fwd(0) == 0  # (rs[:, 2] again the full forward's)
    assert bwd(0) == 0
    torch.cuda.synchronize()
    full = {k: v.clone() for k, v in out.items()}
    for k in ("dpr", "gd", "dp3", "dA", "dp1", "dp2", "part"):
        assert bwd(0, **{k: 1}) == _lib.GMP_ERR_ARG, k
    assert bwd(0, gp_=None) == _lib.GMP_ERR_ARG
    assert bwd(8) == _lib.GMP_ERR_ARG
    assert bwd(NB, dA=1) == _lib.GMP_ERR_ARG and bwd(NG, dp2=1) == _lib.GMP_ERR_ARG
    assert bwd(NB, gd=1) == _lib.GMP_ERR_ARG and bwd(NG, dp3=1) == _lib.GMP_ERR_ARG
    for v in out.values():
        v.fill_(float("nan"))
    assert bwd(NB | NG, gp_=None, amax_=None, dpr=1, gd=1, dp3=1) == 0
    torch.cuda.synchronize()
    for k in ("dA", "dp1", "dp2"):
        assert torch.equal(out[k], full[k]), k
    ln3 = out["part"][:, 4 * d:7 * d]
    assert ln3.abs().max().item() == 0.0 and out["part"][:, 8 * d].abs().max().item() == 0.0
    assert torch.equal(out["part"][:, :4 * d], full["part"][:, :4 * d])
    assert torch.equal(out["part"][:, 7 * d:8 * d], full["part"][:, 7 * d:8 * d])
    assert bwd(NB, gp_=None, dp3=1) == 0 and bwd(NG, dpr=1, gd=1) == 0
    torch.cuda.synchronize()
    assert torch.equal(out["gd"], full["gd"]) and torch.equal(out["dpr"], full["dpr"])
    assert torch.equal(out["dp3"], full["dp3"])
