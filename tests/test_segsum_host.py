"""The model of the in-kernel receiver sums (tests/segsum_ref.py) on the CPU: the wave split is
a partition, the test graphs reach every corner of the mechanism at each kernel's wave count,
the bound helpers reject a dropped and a spurious carry, and a plain fp32 CPU implementation
stays inside every bound that tests/test_gpu_segsum.py applies to the kernels."""
import copy

import pytest
import torch

import segsum_ref as S

CUS = 256  # MI355X; any count >= S.MIN_CUS gives the same wave counts for these graphs
EGNN_CONFIGS = [(128, "swish", "sum"), (128, "relu", "mean"), (32, "swish", "sum")]


@pytest.mark.parametrize("name", S.ALL_GRAPHS)
def test_wave_ranges_partition(name):
    """Node ranges tile [0, N) in order; the edge ranges of the non-empty waves tile [0, E); a
    wave's edges are exactly its receivers' in-edges.  Every n_waves in 1..512."""
    g = S.graph(name)
    for n_waves in range(1, 513):
        node, edge = 0, 0
        for (n_lo, n_hi, e_lo, e_hi) in S.wave_ranges(g.rowptr, n_waves):
            assert n_lo == node and n_hi >= n_lo, (n_waves, n_lo, n_hi)
            node = n_hi
            if n_lo == n_hi:
                assert (e_lo, e_hi) == (0, 0)
                continue
            assert (e_lo, e_hi) == (g.rowptr[n_lo], g.rowptr[n_hi]) and e_lo == edge
            edge = e_hi
        assert node == g.n and edge == g.E, (n_waves, node, edge)


def test_wave_counts():
    """The three launch sizes at 256 CUs, and their independence of the device from 64 CUs on
    for the sizes used here."""
    assert S.egnn_fwd_waves(1, CUS) == 12 and S.egnn_bwd_waves(1, CUS) == 8
    assert S.egnn_fwd_waves(4351, CUS) == 36 and S.egnn_bwd_waves(4351, CUS) == 40
    assert S.egnn_fwd_waves(10 ** 7, CUS) == 256 * 12 and S.egnn_bwd_waves(10 ** 7, CUS) == 256 * 8
    assert S.gvp_waves(1, CUS) == 8 and S.gvp_waves(512, CUS) == 8 and S.gvp_waves(513, CUS) == 16
    assert S.gvp_waves(10 ** 7, CUS) == 256 * 8
    for name in S.ALL_GRAPHS:
        e = S.graph(name).E
        for f in S.WAVE_COUNTS.values():
            assert f(e, S.MIN_CUS) == f(e, CUS) == f(e, 304)


@pytest.mark.parametrize("kernel", sorted(S.WAVE_COUNTS))
def test_graphs_reach_every_situation(kernel):
    """At this kernel's wave count each graph reaches what the GPU tests rely on it for, the new
    graphs together reach every situation, `patterns` alone the carries and the isolated run, and
    the radius graph the suite used so far reaches none of the three it is said to lack."""
    seen = set()
    for name in S.NEW_GRAPHS:
        g = S.graph(name)
        seen |= S.assert_events(g, S.WAVE_COUNTS[kernel](g.E, CUS), kernel)
    assert seen == set(S.SITUATIONS), set(S.SITUATIONS) - seen
    assert set().union(*(S.EXPECT[n] for n in S.NEW_GRAPHS)) == set(S.SITUATIONS)
    assert {"carry_2", "carry_ge9", "end_on_lane15_then_new_segment", "isolated_run_gt64",
            "hub_eats_waves"} <= S.EXPECT["patterns"]
    c = S.graph("control")
    assert not (S.events(c.rowptr, S.WAVE_COUNTS[kernel](c.E, CUS)) & S.CONTROL_LACKS)


def test_graph_builders():
    for name in S.NEW_GRAPHS:
        g = S.graph(name)
        assert g.n <= 700 and g.E <= 6000
        assert not bool((g.edge_index[0] == g.edge_index[1]).any())
        assert bool((g.edge_index >= 0).all()) and bool((g.edge_index < g.n).all())
    p = S.graph("patterns")
    deg = S.degrees(p.recv, p.n)
    assert deg[:len(S.PATTERN_DEGREES)].tolist() == S.PATTERN_DEGREES
    assert int(deg.max()) * 3 > p.E and not bool(deg[-5:].any()) and p.E % 16 != 0
    assert bool((p.recv[1:] < p.recv[:-1]).any())  # shuffled input order
    pairs = p.edge_index[0] * p.n + p.edge_index[1]
    assert pairs.unique().numel() < p.E  # multi-edges
    s = S.graph("star")
    assert int(S.degrees(s.recv, s.n)[0]) == s.n - 1 == int(S.degrees(s.edge_index[0], s.n)[0])
    assert [S.graph(f"tiny{e}").E for e in (1, 15, 16, 17)] == [1, 15, 16, 17]


@pytest.mark.parametrize("kernel", sorted(S.WAVE_COUNTS))
def test_checker_has_teeth(kernel):
    """The fp64 walk reproduces the plain sums; rounded to fp32 it passes the sum and mean
    bounds; the same walk with a first chunk dropped from a multi-chunk segment, or with a
    stale carry added after a chunk that ended on lane 15, is rejected by both."""
    g = S.graph("patterns")
    n_waves = S.WAVE_COUNTS[kernel](g.E, CUS)
    terms = torch.randn(g.E, 8, generator=torch.Generator().manual_seed(1))
    exact, _ = S.model_sum(terms, g.recv, g.n, n_waves)
    deg = S.degrees(g.recv, g.n).clamp(min=1).double().view(-1, 1)
    for mean in (False, True):
        ref, bound = S.sum_bound(terms, g.recv, g.n, mean=mean)
        ok = exact / deg if mean else exact
        assert (ok - ref).abs().max().item() <= 1e-12
        S.assert_within(ok.float(), ref, bound, f"{kernel} exact walk, mean={mean}")
        for fault in ("drop_first_chunk", "spurious_carry"):
            bad, hits = S.model_sum(terms, g.recv, g.n, n_waves, fault=fault)
            assert hits > 0, fault
            bad = bad / deg if mean else bad
            assert S.worst_ratio(bad.float(), ref, bound) > 1.0, (fault, mean)
            with pytest.raises(AssertionError):
                S.assert_within(bad.float(), ref, bound, fault)
    # the zero-row check rejects a row that the zeroing loop missed, and a negative zero
    z = exact.float()
    S.assert_zero_rows(z, g.recv, g.n, "exact")
    for v in (1e-30, -0.0):
        z2 = z.clone()
        z2[-1, 0] = v
        with pytest.raises(AssertionError):
            S.assert_zero_rows(z2, g.recv, g.n, "dirty")


def test_gvp_row_variation_keeps_the_teeth():
    """The allowance for the two kernels' different |vh|^2 (segsum_ref.gvp_row_variation), added
    to the summation bound as the GPU test adds it, still rejects both faulty walks on every
    output row they touch (the smallest margin is printed), and an fp32 CPU evaluation of the layer summed by
    index_add_ passes."""
    from oracle import gvp as ogvp
    g = S.graph("patterns")
    torch.manual_seed(7)
    lay = ogvp.GVP((128, 16), (128, 16), activations=(None, None))
    W = (lay.ws.weight, lay.ws.bias, lay.wsv.weight, lay.wsv.bias, lay.wh.weight, lay.wv.weight)
    gen = torch.Generator().manual_seed(11)
    s, v = torch.randn(g.E, 128, generator=gen), torch.randn(g.E, 16, 3, generator=gen)
    with torch.no_grad():
        rs, rv = lay((s, v))
    n_waves = S.gvp_waves(g.E, CUS)
    for rows, var in zip((rs, rv.reshape(g.E, 48)), S.gvp_row_variation(s, v, W)):
        ref, bound = S.sum_bound(rows, g.recv, g.n)
        bound = bound + S.index_sum(var, g.recv, g.n)
        S.assert_within(torch.zeros(g.n, rows.shape[1]).index_add_(0, g.recv, rows), ref, bound,
                        "fp32 rows, fp32 index_add_")
        for fault in ("drop_first_chunk", "spurious_carry"):
            bad, hits = S.model_sum(rows, g.recv, g.n, n_waves, fault=fault)
            assert hits > 0
            touched = (bad - ref).abs().amax(dim=1) > 0
            worst = ((bad - ref).abs() / bound)[touched].amax(dim=1)
            print(f"{fault}: {int(touched.sum())} rows, smallest worst ratio {worst.min():.3g}")
            assert bool(touched.any()) and float(worst.min()) > 1.0


@pytest.mark.parametrize("name", S.ALL_GRAPHS)
def test_fp32_index_add_within_sum_bounds(name):
    """The CPU's sequential fp32 index_add_ of fp32 rows meets the sum and mean bounds that the
    GVP and CFConv tests apply (rows of the width and scale of those tests' terms)."""
    g = S.graph(name)
    gen = torch.Generator().manual_seed(2)
    terms = torch.randn(g.E, 48, generator=gen) * 3.0
    got = torch.zeros(g.n, 48).index_add_(0, g.recv, terms)
    deg = S.degrees(g.recv, g.n).clamp(min=1).float().view(-1, 1)
    for mean in (False, True):
        ref, bound = S.sum_bound(terms, g.recv, g.n, mean=mean)
        S.assert_within(got / deg if mean else got, ref, bound, f"{name} fp32, mean={mean}")
    S.assert_zero_rows(got, g.recv, g.n, name)
    # CFConv's form: the product rounded once, then summed
    x, w = torch.randn(g.n, 48, generator=gen), torch.randn(g.E, 48, generator=gen)
    j = g.edge_index[0]
    ref, bound = S.sum_bound(x.double()[j] * w.double(), g.recv, g.n, extra=18)
    S.assert_within(torch.zeros(g.n, 48).index_add_(0, g.recv, x[j] * w), ref, bound,
                    f"{name} fp32 products")


@pytest.mark.parametrize("d,act,aggr", EGNN_CONFIGS)
@pytest.mark.parametrize("name", S.ALL_GRAPHS)
def test_fp32_oracle_block_within_egnn_bars(name, d, act, aggr):
    """The fp32 oracle layer's message block against its fp64 copy under the per-row bars of
    the GPU test (1e-5 A_n on m_aggr / pos_aggr, 1e-4 (|ref_n| + median) on dh / dpos, 1e-4 of
    scale on parameter gradients): a correct fp32 implementation stays inside them on these
    inputs.  pos_aggr is the exception the floor exists for (segsum_ref.pos_floor): on `control`
    and the tiny graphs the oracle meets 1e-5 A_n as it stands (floor 0); on `star` and
    `patterns` it misses it on a few rows, every one of them a receiver of ONE edge (one term,
    no sum, no carry), by absolute errors of a few 1e-6 at the most, so the floor stays under the
    project's absolute 1e-5.  The floor reaches single-edge receivers only: every row with two
    or more in-edges is held to exactly 1e-5 A_n, which the oracle meets there."""
    g = S.graph(name)
    ref = S.perturbed_oracle_layer(d, act, aggr, seed=d)
    ref64 = copy.deepcopy(ref).double()
    h, gm, gp = S.egnn_inputs(g, d, seed=d + 1)
    want = S.egnn_block_run(ref64, h, g.pos, g.edge_index, g.n, gm, gp)
    got = S.egnn_block_run(ref, h, g.pos, g.edge_index, g.n, gm, gp)
    floor, rows = S.pos_floor(got, want, g)
    print(f"{name} d={d} {act} {aggr}: pos_aggr floor {floor:.3g}, rows {rows.tolist()}")
    if name not in ("star", "patterns"):
        assert floor == 0.0
    assert floor <= 1e-5
    assert all(d == 1 for d in S.degrees(g.recv, g.n)[rows].tolist())
    S.egnn_check(got, want, g, aggr == "mean", f"{name} fp32 oracle d={d} {act} {aggr}", floor,
                 rows)
    # the floor does not reach a row of two or more in-edges: a wrong value there fails
    multi = torch.nonzero(S.degrees(g.recv, g.n) >= 2).flatten()
    if floor and multi.numel():
        bar = S.row_scale_bound(want["shift"], g.recv, g.n, S.FEATURE_BAR, True).flatten()
        n = int(multi[bar[multi].argmin()])
        bad = dict(got, pos_aggr=got["pos_aggr"].clone())
        bad["pos_aggr"][n, 0] += float(2 * bar[n])  # inside the floor where bar_n < floor / 2
        with pytest.raises(AssertionError):
            S.egnn_check(bad, want, g, aggr == "mean", f"{name} shifted row {n}", floor, rows)


def test_egnn_block_is_the_oracle_layer():
    """On `control` (whose last receiver has an in-edge, as the module needs without dim_size)
    the restated block gives the oracle module's own outputs."""
    g = S.graph("control")
    assert int(S.degrees(g.recv, g.n)[-1]) > 0
    for d, act, aggr in EGNN_CONFIGS:
        lay = S.perturbed_oracle_layer(d, act, aggr, seed=d).double()
        h = S.egnn_inputs(g, d, seed=d + 1)[0].double()
        pos = g.pos.double()
        with torch.no_grad():
            h_new, pos_new = lay(h, pos, g.edge_index)
            m_aggr, p_aggr, _, _ = S.egnn_block(lay, h, pos, g.edge_index, g.n)
            want_h = lay.mlp_upd(torch.cat([h, m_aggr], dim=-1))
        assert (h_new - want_h).abs().max().item() <= 1e-12
        assert (pos_new - (pos + p_aggr)).abs().max().item() <= 1e-12
