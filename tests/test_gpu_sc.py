"""The K8 symmetric-contraction kernels (csrc/gmp_sc.hip: sc_fwd_kernel, sc_bwd_x_kernel,
sc_bwd_coef_kernel) at torch.ops.gmp.symmetric_contraction_{fwd,bwd} against the fp64 evaluation
of the same polynomial (tests/sc_ref.py), at every edge of the launch decomposition: channel
tiles that do not divide 256 or the channel count, one channel, a second grid-stride pass, the
D = 63 and M = 255 caps (opt-in LDS sizes, the term word's sign bit), empty rows and T = 0, every
step of the dcoef kernel's channel tile and its term-block, staging and node-group tails.

Each case builds a synthetic plan (sc_ref.make_plan), passes it through
equivariant.check_k8_plan before any launch, asserts through gmp_sc_route the route fields it is
there for, runs every op twice on freshly dirtied allocations (bitwise equal), and compares out,
dx and part.sum(0) element by element within sc_ref.bound -- (n + 8) 2^-24 of the sum of the
absolute addends, derived in sc_ref's docstring; an element with no addends must be exactly 0.0.
x, coef, gout ~ N(0, 1) from fixed seeds.  Every case prints its error / bound ratios."""
import copy

import pytest
import torch

import sc_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from gmp_amd import _lib
    return _lib.torch_ops()


def _dirty():
    """The next allocations come from a NaN-filled cached block."""
    big = torch.full((1 << 22,), float("nan"), device=DEV)
    del big


def _run(plan_d, M, coef_d, x_d, gout_d):
    _dirty()
    out = _ops().symmetric_contraction_fwd(x_d, plan_d, M, coef_d)
    dx, part = _ops().symmetric_contraction_bwd(x_d, plan_d, M, coef_d, gout_d)
    torch.cuda.synchronize()
    return out, dx, part


def _inputs(M, D, C, T, B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, C, generator=g), torch.randn(B, C, D, generator=g),
            torch.randn(B, M * C, generator=g))


def _case(M, D, C, tpr, B, seed, blocks=None, expect=None):
    """One synthetic case end to end; returns (route, plan, host inputs, GPU outputs, ratios)."""
    from gmp_amd import equivariant as eq
    plan = sc_ref.make_plan(M, D, C, tpr, blocks or sc_ref.blocks_for(M), seed)
    eq.check_k8_plan(plan, M, D, C)
    T = plan.numel() - (3 * M + 1)
    assert B * C * T <= 4e7
    r = sc_ref.route(B, C, D, M, T)
    for k, v in (expect or {}).items():
        assert r[k] == v, (k, r)
    coef, x, gout = _inputs(M, D, C, T, B, seed + 1000)
    dev = [t.to(DEV) for t in (plan, coef, x, gout)]
    got = _run(dev[0], M, *dev[1:])
    again = _run(dev[0], M, *dev[1:])
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs differ"
    out, dx, part = got
    assert out.shape == (B, M * C) and dx.shape == (B, C, D) and part.shape == (r["G"], T, C)
    ref = sc_ref.eval_plan64(plan, M, coef, x, gout,
                             n_dcoef=r["nodes_per_group"] + r["G"])
    q = sc_ref.ratios(ref, out, dx, part.sum(0))
    print(f"K8 M={M} D={D} C={C} T={T} B={B}: error / bound "
          f"out {q['out']:.3f} dx {q['dx']:.3f} dcoef {q['dcoef']:.3f}")
    assert max(q.values()) < 1.0, (q, r)
    return r, plan, (coef, x, gout), got, q


@pytest.mark.parametrize("C,npb", [(3, 85), (5, 51)])
def test_idle_threads(C, npb):
    """256 % CT != 0: threads past npb CT idle; B around one pass of a workgroup."""
    for B in (1, npb - 1, npb, npb + 1):
        _case(4, 4, C, 5, B, seed=10 * C + B % 7, expect=dict(CT=C, npb=npb, channel_tiles=1))


@pytest.mark.parametrize("C,tiles", [(17, 2), (33, 3)])
def test_partly_filled_last_channel_tile(C, tiles):
    _case(9, 9, C, [7, 6, 7, 6, 7, 6, 7, 7, 7], 100, seed=C,
          expect=dict(CT=16, npb=16, channel_tiles=tiles))


def test_single_channel():
    _case(4, 4, 1, 5, 257, seed=3, expect=dict(CT=1, npb=256, channel_tiles=1, CT_d=1))


def test_second_grid_stride_pass():
    """More nodes than node_blocks npb: workgroup 0 takes a full second pass of the grid-stride
    loop, workgroup 1 a second pass of one node."""
    probe = sc_ref.route(1 << 30, 16, 4, 4, 12)
    nblk, npb = probe["node_blocks"], probe["npb"]
    assert npb == 16 and nblk == 8 * torch.cuda.get_device_properties(0).multi_processor_count
    B = nblk * npb + npb + 1
    _case(4, 4, 16, 3, B, seed=4, expect=dict(node_blocks=nblk, npb=16, channel_tiles=1))


def test_dim_cap_lds_opt_in():
    """D = 63: 66,560 B (forward) and 133,120 B (dx) of dynamic LDS, past the 64 KiB default."""
    _case(9, 63, 16, [14, 13, 13, 14, 13, 13, 14, 13, 13], 64, seed=5,
          expect=dict(lds_fwd=66_560, lds_dx=133_120, CT=16))


def test_dim_one():
    """D = 1: x_0 .. x_0^4 in each of two rows."""
    r, plan, _, _, _ = _case(2, 1, 4, 4, 50, seed=6, blocks=[1, 1])
    fac = sc_ref.split_plan(plan, 2)[3]
    assert sorted((fac == 0).sum(1).tolist()) == [1, 1, 2, 2, 3, 3, 4, 4]


def test_row_field_sign_bit_and_row_cap():
    """M = 255: rows 128.. set the term word's sign bit."""
    tpr = [1 + (m * 7) % 3 for m in range(255)]
    r, plan, _, _, _ = _case(255, 9, 4, tpr, 40, seed=7)
    assert int((plan[3 * 255 + 1:] < 0).sum()) == sum(tpr[128:])


def test_row_cap_at_dim_cap_staging():
    """M = 255 with D = 63 and C = 16: the dcoef kernel stages NB = 3 nodes per round (one term
    per row keeps T <= 256, so CT_d stays 16)."""
    _case(255, 63, 16, 1, 40, seed=8, expect=dict(NB=3, CT_d=16, lds_fwd=66_560))


def test_rows_without_terms():
    """Rows 0, 4 and 8 hold no terms: their output columns are exactly 0.0 on a dirty buffer."""
    M, C = 9, 4
    r, plan, _, (out, dx, part), _ = _case(M, 9, C, [0, 5, 5, 5, 0, 5, 5, 5, 0], 100, seed=9)
    _, base, stride, _, _ = sc_ref.split_plan(plan, M)
    for m in (0, 4, 8):
        cols = int(base[m]) + int(stride[m]) * torch.arange(C)
        assert torch.equal(out[:, cols.to(DEV)], torch.zeros(100, C, device=DEV)), m


@pytest.mark.parametrize("B", [40, 700])
def test_no_terms(B):
    """T = 0: out and dx exactly zero, part (G, 0, C)."""
    r, _, _, (out, dx, part), _ = _case(4, 4, 4, 0, B, seed=11, expect=dict(z_blocks=0))
    assert torch.equal(out, torch.zeros_like(out)) and torch.equal(dx, torch.zeros_like(dx))
    assert part.shape == (r["G"], 0, 4)


@pytest.mark.parametrize("T,ctd", [(1, 16), (256, 16), (257, 15), (273, 15), (586, 6)])
def test_dcoef_channel_tile_steps(T, ctd):
    """CT_d = clamp(4096 // T, 1, 16) at C = 17: a last tile of 1 (CT_d 16), 2 (15) or 5 (6)
    channels, and pair indices p = term CT_d + channel with CT_d not a power of two."""
    M = 9
    tpr = [T // M + (1 if m < T % M else 0) for m in range(M)]
    _case(M, 9, 17, tpr, 70, seed=12 + T, expect=dict(CT_d=ctd, terms_per_wg=4096 // ctd,
                                                     z_blocks=1))


@pytest.mark.parametrize("T,zb", [(4096, 1), (4097, 2)])
def test_dcoef_one_channel_per_tile_and_z_tail(T, zb):
    """T >= 4096: one channel per tile; T = 4097: a second term block that holds one term."""
    M = 16
    tpr = [T // M + (1 if m < T % M else 0) for m in range(M)]
    _case(M, 16, 3, tpr, 40, seed=13 + T, expect=dict(CT_d=1, terms_per_wg=4096, z_blocks=zb))


@pytest.mark.parametrize("B", [70, 5])
def test_dcoef_staging_tail(B):
    """NB = 32 staged nodes per round: a last round of 70 % 32 = 6 nodes, and B = 5 < NB."""
    r, *_ = _case(4, 4, 4, 4, B, seed=14 + B, expect=dict(NB=32, G=1, nodes_per_group=B))
    assert r["nodes_per_group"] % r["NB"] != 0


@pytest.mark.parametrize("B,G,per", [(256, 1, 256), (257, 2, 129), (32_768, 128, 256),
                                     (32_769, 128, 257)])
def test_group_edges(B, G, per):
    """One group to two, and the 128-group cap with 256 and 257 nodes per group (the last group
    of B = 32,769 holds 130)."""
    _case(4, 4, 4, 4, B, seed=15 + B % 11, expect=dict(G=G, nodes_per_group=per))


# ----------------------------------------------------------------------------- exact properties
def test_large_batch_rows_and_groups_equal_their_own_runs():
    """B = 33,000, C = 17: rows [a, b) of out and dx equal the run on x[a:b] alone; B = 32,768:
    part[g] equals part[0] of a run on that group's nodes alone (fixed summation order per (node,
    channel) and per (term, channel, group)): torch.equal."""
    from gmp_amd import equivariant as eq
    M, D, C, B = 9, 9, 17, 33_000
    plan = sc_ref.make_plan(M, D, C, 7, sc_ref.blocks_for(M), seed=21)
    eq.check_k8_plan(plan, M, D, C)
    T = plan.numel() - (3 * M + 1)
    r = sc_ref.route(B, C, D, M, T)
    G, per = r["G"], r["nodes_per_group"]
    assert (G, per) == (128, 258) and B > r["node_blocks"] * r["npb"]
    coef, x, gout = _inputs(M, D, C, T, B, 22)
    plan_d, coef_d, x_d, gout_d = (t.to(DEV) for t in (plan, coef, x, gout))
    out, dx, part = _run(plan_d, M, coef_d, x_d, gout_d)
    assert all(torch.equal(a, b) for a, b in
               zip((out, dx, part), _run(plan_d, M, coef_d, x_d, gout_d)))
    for a, b in ((0, 300), (12_345, 13_045), (B - 17, B)):
        o2, d2, _ = _run(plan_d, M, coef_d, x_d[a:b].contiguous(), gout_d[a:b].contiguous())
        assert torch.equal(out[a:b], o2) and torch.equal(dx[a:b], d2), (a, b)
    # a group of 258 nodes run alone would split into two groups of its own, so the group
    # property is taken at B = 32,768: exactly 256 nodes in each of 128 groups
    B2 = 32_768
    _, _, part2 = _run(plan_d, M, coef_d, x_d[:B2].contiguous(), gout_d[:B2].contiguous())
    assert part2.shape[0] == 128
    for g in (0, 1, 77, 127):
        a, b = g * 256, (g + 1) * 256
        _, _, p2 = _run(plan_d, M, coef_d, x_d[a:b].contiguous(), gout_d[a:b].contiguous())
        assert p2.shape[0] == 1 and torch.equal(part2[g], p2[0]), g


# ------------------------------------------------------------------------------- real modules
def test_large_batch_gradients_on_a_real_plan():
    """4x0e+4x1o+4x2e at correlation 3, B = 33,000 (128 groups of 258 nodes): out, dx and dcoef
    against eval_plan64 on the module's plan and k8_coefficients()."""
    from gmp_amd import equivariant as eq
    torch.manual_seed(31)
    irr = "4x0e+4x1o+4x2e"
    sc = eq.SymmetricContraction(irr, irr, 3)
    assert sc._k8
    M, C, D, B = sc._k8_rows, 4, 9, 33_000
    plan = sc._k8_plan
    eq.check_k8_plan(plan, M, D, C)
    with torch.no_grad():
        coef = sc.k8_coefficients().contiguous()
    T = coef.shape[0]
    assert B * C * T <= 4e7
    r = sc_ref.route(B, C, D, M, T)
    assert (r["G"], r["nodes_per_group"]) == (128, 258)
    _, x, gout = _inputs(M, D, C, T, B, 32)
    dev = [t.to(DEV) for t in (coef, x, gout)]
    out, dx, part = _run(plan.to(DEV), M, *dev)
    assert all(torch.equal(a, b) for a, b in zip((out, dx, part), _run(plan.to(DEV), M, *dev)))
    ref = sc_ref.eval_plan64(plan, M, coef, x, gout, n_dcoef=r["nodes_per_group"] + r["G"])
    q = sc_ref.ratios(ref, out, dx, part.sum(0))
    print(f"K8 real plan M={M} D={D} C={C} T={T} B={B}: error / bound "
          f"out {q['out']:.3f} dx {q['dx']:.3f} dcoef {q['dcoef']:.3f}")
    assert max(q.values()) < 1.0, q


@pytest.mark.parametrize("irr,corr", [("20x0e+20x1o+20x2e", 3), ("3x0e+3x1o", 4)])
def test_module_vs_fp64_oracle(irr, corr):
    """Through the module (k8_coefficients' fold and gather at a channel tail: C = 20 is a tile of
    16 and one of 4, C = 3 one of 3) against the fp64 oracle.  out and dx within sc_ref.bound
    evaluated on the module's plan and its fp32 coefficients; weight gradients within 1e-5 of
    each gradient's scale plus twice the fp32 oracle's own distance from fp64."""
    from gmp_amd import equivariant as eq
    from oracle import mace as om
    torch.manual_seed(40 + corr)
    ref32 = om.SymmetricContraction(irr, irr, corr)
    ref64 = copy.deepcopy(ref32).double()
    sc = eq.SymmetricContraction(irr, irr, corr)
    sc.load_state_dict(ref32.state_dict())
    assert sc._k8
    C = int(irr.split("x")[0])
    D = sum(2 * int(t.split("x")[1][:-1]) + 1 for t in irr.split("+"))
    M, B = sc._k8_rows, 300
    eq.check_k8_plan(sc._k8_plan, M, D, C)
    g = torch.Generator().manual_seed(41)
    x, gout = torch.randn(B, C, D, generator=g), torch.randn(B, M * C, generator=g)
    with torch.no_grad():
        coef = sc.k8_coefficients().contiguous()
    T = coef.shape[0]
    assert B * C * T <= 4e7
    bnd = sc_ref.eval_plan64(sc._k8_plan, M, coef, x, gout, n_dcoef=B + 1)
    sc = sc.to(DEV)
    xd = x.clone().to(DEV).requires_grad_(True)
    _dirty()
    y = sc(xd)
    (y * gout.to(DEV)).sum().backward()
    x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    (ref32(x32) * gout).sum().backward()
    y64 = ref64(x64)
    (y64 * gout.double()).sum().backward()
    q_out = sc_ref.ratio(y, y64.detach(), bnd["n_out"], bnd["S_out"])
    q_dx = sc_ref.ratio(xd.grad, x64.grad, bnd["n_dx"], bnd["S_dx"])
    print(f"K8 module {irr} corr {corr} T={T}: error / bound out {q_out:.3f} dx {q_dx:.3f}")
    worst = 0.0
    for (k, p), p32, p64 in zip(sc.named_parameters(), ref32.parameters(), ref64.parameters()):
        err = (p.grad.cpu().double() - p64.grad).abs().max().item()
        err32 = (p32.grad.double() - p64.grad).abs().max().item()
        scale = p64.grad.abs().max().item()
        worst = max(worst, err / (1e-5 * scale + 2 * err32 + 1e-300))
        assert err <= 1e-5 * scale + 2 * err32, (k, err, err32, scale)
    print(f"K8 module {irr} corr {corr}: worst weight-gradient error / allowance {worst:.3f}")
    assert q_out < 1.0 and q_dx < 1.0, (q_out, q_dx)
