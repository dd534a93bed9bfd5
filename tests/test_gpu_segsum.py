"""The receivers' sums that four edge kernels do themselves (egnn_fwd_kernel, egnn_bwd_kernel,
gvp_layer_fwd_agg_kernel, gvp_msg0_bwd_agg_kernel) against fp64 at the degree edges: carries
over many chunks, a stale carry that must not be taken, 16 degree-1 receivers in a chunk, a hub
that swallows several waves' targets, runs of isolated receivers, ranges shorter than a chunk,
E in {1, 15, 16, 17}.  tests/segsum_ref.py models the mechanism; every test first asserts, from
the wave count its launch uses, that its graph reaches the situations it is there for
(segsum_ref.EXPECT; tests/test_segsum_host.py shows that together they are all of them).  K13's
two-rows-in-flight loop rides along on the same graphs.

Bounds: sums of identical fp32 rows in another order get the summation bound
(deg + 16) 2^-23 sum |t| (segsum_ref.sum_bound); the EGNN block, whose per-edge rows are not
available outside the kernel, gets the project's 1e-5 / 1e-4 bars per row (segsum_ref.egnn_check
and DESIGN.md section 5)."""
import copy

import pytest
import torch

import segsum_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
EGNN_GRAPHS = ("patterns", "star", "tiny1", "tiny17", "control")


def _cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    if n < S.MIN_CUS:
        pytest.skip(f"{n} CUs: the wave counts of tests/segsum_ref.py hold from {S.MIN_CUS} on")
    return n


def _gvp_weights():
    import gmp_amd.gvp as gvp
    torch.manual_seed(7)
    lay = gvp.GVP((128, 16), (128, 16), activations=(None, None)).to(DEV)
    return (lay.ws.weight, lay.ws.bias, lay.wsv.weight, lay.wsv.bias, lay.wh.weight, lay.wv.weight)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("name", S.ALL_GRAPHS)
def test_gvp_layer_agg_vs_fp64(name, reduce):
    """GvpLayerAggFn against the unfused GvpLayerFn's per-edge rows summed in fp64.

    The fused kernel's per-edge rows are NOT those of gvp_layer_fwd_x3_kernel bit for bit.  Both
    call layer_forward_x3<false> on the same LDS image and form the gate product with the same
    single multiplication, but vnorm's x^2 + y^2 + z^2 is left to the compiler's contraction,
    and the two kernels' code objects hold different forms of it (fma(z, z, fma(y, y, x x))
    against a packed multiply, an fma and an add), so vn, and through Ws and the gate every
    output, may differ in the last bits.  segsum_ref.gvp_row_variation derives the bound of
    that difference from the inputs; it is added per edge to the summation bound.
    Sum: (deg + 16) 2^-23 sum |t| + sum of the rows' variation, per row and component; mean:
    that over deg plus 2^-23 |ref|; isolated rows exactly +0.  Input and weight gradients
    bitwise those of the unfused pair."""
    import gmp_amd.gvp as gvp
    from gmp_amd import ops
    g = S.graph(name)
    S.assert_events(g, S.gvp_waves(g.E, _cus()), "gvp_layer_fwd_agg_kernel")
    W = _gvp_weights()
    csr = ops.get_csr(g.recv.to(DEV), g.n)
    gen = torch.Generator().manual_seed(11)
    s, v = torch.randn(g.E, 128, generator=gen).to(DEV), torch.randn(g.E, 16, 3, generator=gen).to(DEV)
    gs, gv = torch.randn(g.n, 128, generator=gen).to(DEV), torch.randn(g.n, 16, 3, generator=gen).to(DEV)
    outs = []
    for fused in (True, False):
        for p in W:
            p.grad = None
        sd, vd = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
        if fused:
            a_s, a_v = gvp.GvpLayerAggFn.apply(sd, vd, *W, csr, reduce)
        else:
            s3, v3 = gvp.GvpLayerFn.apply(sd, vd, *W, False)
            a_s = ops.SegmentReduceFn.apply(s3, csr, reduce)
            a_v = ops.SegmentReduceFn.apply(v3.reshape(g.E, 48), csr, reduce).view(g.n, 16, 3)
        ((a_s * gs).sum() + (a_v * gv).sum()).backward()
        torch.cuda.synchronize()
        outs.append([a_s.detach(), a_v.detach(), sd.grad, vd.grad] + [p.grad.clone() for p in W])
    rows_s, rows_v = s3.detach().cpu(), v3.detach().reshape(g.E, 48).cpu()
    a_s, a_v = outs[0][0].cpu(), outs[0][1].reshape(g.n, 48).cpu()
    assert a_s.shape == (g.n, 128) and outs[0][1].shape == (g.n, 16, 3)
    var_s, var_v = S.gvp_row_variation(s, v, W)
    for got, rows, var, what in ((a_s, rows_s, var_s, "s"), (a_v, rows_v, var_v, "v")):
        ref, bound = S.sum_bound(rows, g.recv, g.n, mean=reduce == "mean")
        extra = S.index_sum(var, g.recv, g.n)
        if reduce == "mean":
            extra = extra / S.degrees(g.recv, g.n).clamp(min=1).double().view(-1, 1)
        S.assert_within(got, ref, bound + extra, f"{name} {reduce} {what}_agg")
        S.assert_zero_rows(got, g.recv, g.n, f"{name} {what}_agg isolated rows")
    for k, (a, b) in enumerate(zip(outs[0][2:], outs[1][2:])):
        assert torch.equal(a, b), f"{name} {reduce}: gradient {k} differs from the unfused pair"


@pytest.mark.parametrize("name", S.ALL_GRAPHS)
def test_gvp_msg0_bwd_agg_vs_fp64(name):
    """gmp_gvp_msg0_bwd_agg_f32: per-edge outputs bitwise those of gmp_gvp_msg0_bwd_f32; the
    receiver sums dPb = S dspre, dQb = S dvh, S dgate, S dvpre within (deg + 16) 2^-23 sum |t|
    of the fp64 sums of those per-edge rows; isolated rows exactly +0."""
    from gmp_amd import _lib, ops
    tops = _lib.torch_ops()
    g = S.graph(name)
    S.assert_events(g, S.gvp_waves(g.E, _cus()), "gvp_msg0_bwd_agg_kernel")
    n, E = g.n, g.E
    gen = torch.Generator().manual_seed(5)

    def rn(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(DEV)

    send, recv = (g.edge_index[k].to(DEV).contiguous() for k in (0, 1))
    rcsr = ops.get_csr(recv, n)
    P, Q, es, ev = rn(n, 256), rn(n, 288), rn(E, 32), rn(E, 3)
    W = [rn(128, 32, scale=0.2), rn(128, 48, scale=0.2), rn(128), rn(16, 48, scale=0.2),
         rn(16, 128, scale=0.1), rn(16), rn(48, scale=0.3)]
    ds, dv = rn(E, 128), rn(E, 48)
    ref = tops.gvp_msg0_bwd(send, recv, P, Q, es, ev, W, ds, dv, False)
    got = tops.gvp_msg0_bwd_agg(send, recv, P, Q, es, ev, W, ds, dv, rcsr.perm, rcsr.rowptr, n,
                                False)
    torch.cuda.synchronize()
    for k in (0, 2, 3, 5, 6, 7, 8):
        assert torch.equal(got[k], ref[k]), f"{name}: per-edge output {k}"
    for k, src, what in ((9, ref[0], "dPb"), (10, ref[6], "dQb"), (11, ref[2], "S dgate"),
                         (12, ref[5], "S dvpre")):
        rows = src.reshape(E, -1).cpu()
        out = got[k].reshape(n, -1).cpu()
        want, bound = S.sum_bound(rows, g.recv, n)
        S.assert_within(out, want, bound, f"{name} {what}")
        S.assert_zero_rows(out, g.recv, n, f"{name} {what} isolated rows")


@pytest.mark.parametrize("d,act,aggr", [(128, "swish", "sum"), (128, "relu", "mean"),
                                        (32, "swish", "sum")])
@pytest.mark.parametrize("name", EGNN_GRAPHS)
def test_egnn_message_block_vs_fp64(name, d, act, aggr):
    """ops.EgnnMessageFn (EGNNLayer.fused_message: egnn_fwd_kernel, egnn_bwd_kernel) with the
    default HF products and with gmp_egnn_set_f32_mfma(1), against the fp64 restatement of the
    oracle layer's message block with dim_size = N (segsum_ref.egnn_block; on `control`
    tests/test_segsum_host.py asserts that it is the oracle module).

    m_aggr and pos_aggr: row n within 1e-5 A_n, A_n = sum over its in-edges of max_f |row| (over
    deg for a mean; pos_aggr is always a mean), isolated rows exactly +0; dh, dpos: row n within
    1e-4 (|ref_n|_inf + median_n |ref_n|_inf); parameters: 1e-4 of scale + 1e-6.  The pos_aggr
    rows of single-edge receivers, and no others, have the floor of segsum_ref.pos_floor, taken
    from the fp32 CPU oracle on the same inputs (0 on `control` and the tiny graphs; a few 1e-6
    absolute on `star` and `patterns`, where the shift scalar of some single edges cancels);
    every row with two or more in-edges, the hubs included, keeps exactly 1e-5 A_n.  In addition HF stays within 2 x the f32 path's error + 1e-6
    of scale on every output."""
    import gmp_amd
    from gmp_amd import _lib
    lib = _lib.load()
    g = S.graph(name)
    cus = _cus()
    S.assert_events(g, S.egnn_fwd_waves(g.E, cus), "egnn_fwd_kernel")
    S.assert_events(g, lib.gmp_egnn_edge_bwd_partials_rows(g.E, d) * S.BWD_WAVES, "egnn_bwd_kernel")
    assert lib.gmp_egnn_edge_bwd_partials_rows(g.E, d) * S.BWD_WAVES == S.egnn_bwd_waves(g.E, cus)
    ref = S.perturbed_oracle_layer(d, act, aggr, seed=d)
    ref64 = copy.deepcopy(ref).double()
    h, gm, gp = S.egnn_inputs(g, d, seed=d + 1)
    want = S.egnn_block_run(ref64, h, g.pos, g.edge_index, g.n, gm, gp)
    floor, missed = S.pos_floor(S.egnn_block_run(ref, h, g.pos, g.edge_index, g.n, gm, gp), want,
                                g)
    # the floor is confined to single-edge receivers (egnn_check asserts it again per call)
    assert floor <= S.FEATURE_BAR and bool((S.degrees(g.recv, g.n)[missed] == 1).all())
    if name not in ("star", "patterns"):
        assert floor == 0.0
    ei = g.edge_index.to(DEV)

    def run(f32):
        prev = lib.gmp_egnn_set_f32_mfma(f32)
        try:
            lay = gmp_amd.EGNNLayer(d, act, "layer", aggr)
            lay.load_state_dict(ref.state_dict())
            lay = lay.to(DEV)
            hd, pd = h.to(DEV).requires_grad_(True), g.pos.to(DEV).requires_grad_(True)
            assert lay.fused_supported(hd, pd)
            m_aggr, p_aggr = lay.fused_message(ei, hd, pd)
            ((m_aggr * gm.to(DEV)).sum() + (p_aggr * gp.to(DEV)).sum()).backward()
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().cpu() for k, p in lay.named_parameters()
                     if k.startswith(S.BLOCK_PARAMS)}
            return dict(m_aggr=m_aggr.detach().cpu(), pos_aggr=p_aggr.detach().cpu(),
                        dh=hd.grad.cpu(), dpos=pd.grad.cpu(), grads=grads)
        finally:
            lib.gmp_egnn_set_f32_mfma(prev)

    tag = f"{name} d={d} {act} {aggr}"
    e_f32 = S.egnn_check(run(1), want, g, aggr == "mean", tag + " f32", floor, missed)
    e_hf = S.egnn_check(run(0), want, g, aggr == "mean", tag + " HF", floor, missed)
    scales = dict(want["grads"], **{k: want[k] for k in ("m_aggr", "pos_aggr", "dh", "dpos")})
    for k, e in e_hf.items():
        scale = scales[k].abs().max().item() + 1e-30
        assert e <= 2 * e_f32[k] + 1e-6 * scale, (tag, k, e, e_f32[k], scale)


@pytest.mark.parametrize("F", [4, 128, 260])
@pytest.mark.parametrize("name", ["patterns", "star"])
def test_cfconv_aggregate_vs_fp64(name, F):
    """K13 cfconv_gather_mul_sum, plain and escale-scaled, over the receiver CSR and over the
    sender CSR (the form the backward uses), against the fp64 sum of x[src] * w: within
    (deg + 18) 2^-23 sum |x w| (the summation bound with the product's one rounding added).
    F = 4 puts 64 rows in flight per pass, so only segments of more than 64 edges (the hubs of
    these graphs) enter the two-row loop; F = 128 (2 rows) meets the degrees 0..3 of `patterns`
    and `star`; F = 260 takes the column loop."""
    from gmp_amd import ops
    g = S.graph(name)
    deg = S.degrees(g.recv, g.n)
    assert int(deg.max()) > 2 * 64 and (name != "patterns" or {0, 1, 2, 3} <= set(deg.tolist()))
    gen = torch.Generator().manual_seed(F)
    x, w = torch.randn(g.n, F, generator=gen), torch.randn(g.E, F, generator=gen)
    es = torch.rand(g.E, generator=gen) + 0.5
    send, recv = g.edge_index[0], g.edge_index[1]
    xd, wd, esd = x.to(DEV), w.to(DEV), es.to(DEV)
    for gather, seg, what in ((send, recv, "receiver CSR"), (recv, send, "sender CSR")):
        csr = ops.get_csr(seg.to(DEV).contiguous(), g.n)
        for scale, tag in ((None, "plain"), (esd, "escale")):
            y = ops.cfconv_aggregate(xd, gather.to(DEV).contiguous(), wd, csr, scale)
            torch.cuda.synchronize()
            terms = x.double()[gather] * w.double()
            if scale is not None:
                terms = terms * es.double().view(-1, 1)
            ref, bound = S.sum_bound(terms, seg, g.n, extra=18)
            S.assert_within(y.cpu(), ref, bound, f"{name} F={F} {what} {tag}")
            S.assert_zero_rows(y.cpu(), seg, g.n, f"{name} F={F} {what} {tag} isolated rows")
