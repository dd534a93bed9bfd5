"""Host side of the z / dz kernel tests (no GPU): the fp64 reference tests/tp_z_ref.py is pinned
against oracle.o3.FullyConnectedTensorProduct, so it is independent of the code under test; the
plan list of tests/test_gpu_tp_z.py is shown to reach every route the kernels choose among
(tp_z_ref.z_route); and TPPlan refuses spherical-harmonics irreps that are not l = 0..L in
order, which the z / dz kernels (SH component l2 * l2 + j) would misread."""
import pytest
import torch

import test_gpu_tp_z as gz
import tp_z_ref as zref
from oracle import o3 as oo3


def _plan(irreps_in, lmax, irreps_out):
    from gmp_amd import equivariant, o3
    return equivariant.TPPlan(o3.parse_irreps(irreps_in), o3.sh_irreps(lmax),
                              o3.parse_irreps(irreps_out))


_BOTH = "3x0e+3x0o+3x1e+3x1o+3x2e+3x2o"
PIN = [("4x0e+4x1o+4x2e", 2, "4x0e+4x1o+4x2e"),                      # l <= 2, plain
       (_BOTH, 2, _BOTH.replace("3x", "2x")),                        # both parities
       ("3x0e+3x1o+3x2e+3x3o", 3, "3x0e+3x1o+3x2e+3x3o"),            # max_ell = 3
       ("2x0e+2x1o+2x2e+2x3o+2x4e", 4, "2x0e+2x1o+2x2e+2x3o+2x4e")]  # max_ell = 4


@pytest.mark.parametrize("irreps_in,lmax,irreps_out", PIN)
def test_reference_matches_oracle(irreps_in, lmax, irreps_out):
    """z_ref contracted with per-edge weights, out[e, io][w, k] += sum_u W_e[p][u, w] z_p[e][u, k],
    is the oracle's FullyConnectedTensorProduct to 1e-12 of each entry's sum of absolute terms.
    The CG tensors here are the unrounded float64 ones (an fp32 table cannot meet 1e-12); the
    table the kernels read, which z_ref uses by default, must be exactly their fp32 rounding."""
    plan = _plan(irreps_in, lmax, irreps_out)
    cg = zref.cg_f64(plan)
    assert torch.equal(plan.cg_host, cg.float())
    tp = oo3.FullyConnectedTensorProduct(irreps_in, oo3.spherical_harmonics_irreps(lmax),
                                         irreps_out)
    assert tp.weight_numel == plan.weight_numel
    g = torch.Generator().manual_seed(lmax + len(irreps_in))
    N, E, e0, e1 = 7, 24, 3, 19
    x = torch.randn(N, plan.in_dim, generator=g, dtype=torch.float64)
    sh = torch.randn(E, plan.sh_dim, generator=g, dtype=torch.float64)
    W = torch.randn(e1 - e0, plan.weight_numel, generator=g, dtype=torch.float64)
    src, perm = torch.randint(0, N, (E,), generator=g), torch.randperm(E, generator=g)
    want = tp(x[src[e0:e1]], sh[perm[e0:e1]], W)
    a = (plan, x, sh, src, perm, e0, e1, cg)
    outs = []
    for zs, Wq in ((zref.z_ref(*a), W), (zref.z_abs(*a), W.abs())):
        out = torch.zeros(e1 - e0, plan.out_dim, dtype=torch.float64)
        for P, ins, z in zip(zref.paths(plan), plan.instructions, zs):
            m1, mo, d3 = P["mul1"], ins["mul_out"], 2 * P["lo"] + 1
            Wp = Wq[:, ins["w_off"]:ins["w_off"] + m1 * mo].view(-1, m1, mo)
            off = plan.blocks[P["io"]][0]
            out[:, off:off + mo * d3] += torch.einsum("euw,eku->ewk", Wp,
                                                      z.view(-1, d3, m1)).reshape(e1 - e0, -1)
        outs.append(out)
    got, scale = outs
    assert scale.min() > 0
    assert ((got - want).abs() <= 1e-12 * scale).all(), ((got - want).abs() / scale).max()


def test_dz_ref_is_the_adjoint_of_z_ref():
    """<dz, z(x, sh)> differentiated by autograd gives dz_ref's dx_edge / dY_edge (per edge:
    senders and SH rows taken one per edge), so the hand contraction is the same bilinear map."""
    plan = _plan("3x0e+2x0o+3x1o+2x2e", 2, "2x0e+2x1o+2x2e")
    g = torch.Generator().manual_seed(5)
    ne = 6
    x = torch.randn(ne, plan.in_dim, generator=g, dtype=torch.float64, requires_grad=True)
    sh = torch.randn(ne, plan.sh_dim, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.arange(ne)
    zs = zref.z_ref(plan, x, sh, idx, idx, 0, ne)
    dz = [torch.randn(z.shape, generator=g, dtype=torch.float64) for z in zs]
    sum((z * d).sum() for z, d in zip(zs, dz)).backward()
    dx, dY, dxa, dYa = zref.dz_ref(plan, x.detach(), sh.detach(), idx, idx, 0, ne, dz)
    torch.testing.assert_close(dx, x.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dY, sh.grad, rtol=1e-12, atol=1e-13)
    route = zref.z_route(plan)
    assert route["uncovered"] == 2 and (dx[:, 3:5] == 0).all() and (dxa[:, 3:5] == 0).all()
    assert (dxa >= dx.abs()).all() and (dYa >= dY.abs()).all()


def test_plan_list_reaches_every_route():
    routes = {p[0]: zref.z_route(gz.make_plan(p[0])) for p in gz.PLANS}
    plans = {p[0]: gz.make_plan(p[0]) for p in gz.PLANS}

    def some(pred):
        return [n for n, r in routes.items() if pred(r, plans[n])]

    kernels = ("z2<2>", "z2<3>", "gen")
    assert some(lambda r, p: r["kernel"] == "z2<2>" and r["pre"])
    assert some(lambda r, p: r["kernel"] == "z2<2>" and r["grouped"] and not r["pre"])
    assert some(lambda r, p: r["kernel"] == "z2<3>" and not r["grouped"] and r["l1_max"] == 3)
    assert some(lambda r, p: r["kernel"] == "z2<3>" and r["grouped"] and r["l1_max"] == 3)
    assert some(lambda r, p: r["kernel"] == "z2<3>" and p.sh_dim == 9)
    assert some(lambda r, p: r["kernel"] == "gen" and p.l_max > 3)
    assert some(lambda r, p: r["kernel"] == "gen" and p.sh_dim == 25 and p.l_max <= 2)
    assert some(lambda r, p: r["kernel"] == "gen" and p.sh_dim == 25 and p.l_max == 4 and
                max(l for _, (l, _) in p.irreps_in + p.irreps_out) == 2)
    assert some(lambda r, p: r["kernel"] == "gen" and r["grouped"])
    for k in kernels:
        assert some(lambda r, p: r["kernel"] == k and r["uncovered"] > 0), k
        assert some(lambda r, p: r["kernel"] == k and "partial" in r["mul_halves"].values()), k
        assert some(lambda r, p: r["kernel"] == k and 128 in r["mul_halves"]), k
    assert some(lambda r, p: r["ragged"])
    # pre is a forward decision of the LM = 2 kernel alone
    assert not some(lambda r, p: r["pre"] and (r["kernel"] != "z2<2>" or r["grouped"]))
    # what the issue's table states of single plans
    assert routes["z2_uncovered_24"]["uncovered"] == 24
    assert routes["z3_grouped_34"]["uncovered"] == 4 and routes["z3_grouped_34"]["n_paths"] == 34
    assert routes["z3_uncovered_56"]["uncovered"] == 56
    assert routes["z3_uncovered_56"]["kernel"] == "z2<3>" and plans["z3_uncovered_56"].l_max == 2
    assert routes["gen_l4_42"]["n_paths"] == 42 and plans["gen_l4_42"].cg_host.numel() == 7194
    assert routes["gen_grouped"]["uncovered"] == 4
    assert routes["ragged_65_127_3"]["mul_halves"] == {65: "partial", 127: "partial", 3: "one"}
    assert plans["sh1_one_path"].sh_dim == 1 and routes["sh1_one_path"]["n_paths"] == 1


@pytest.mark.parametrize("sh", ["1x1o+1x0e", "1x0e+1x2e+1x1o", "1x0e+1x2e", "1x0e+1x0o+1x1o+1x1e",
                                "2x0e", "1x1o", "1x0e+1x1o+1x3o+1x2e"])
def test_sh_order_is_refused(sh):
    """"1x1o+1x0e" was accepted before (y_off 0 for l2 = 1, 3 for l2 = 0) and the node form would
    have read the wrong SH components."""
    from gmp_amd import equivariant, o3
    io = o3.parse_irreps("8x0e+8x1o")
    with pytest.raises(NotImplementedError):
        equivariant.TPPlan(io, o3.parse_irreps(sh), io)


@pytest.mark.parametrize("L", range(6))
def test_sh_irreps_still_build(L):
    from gmp_amd import equivariant, o3
    hid = o3.hidden_irreps(2, min(L, 1))   # (every l up to 5 on both sides: more than 48 paths)
    plan = equivariant.TPPlan(hid, o3.sh_irreps(L), o3.hidden_irreps(2, L))
    assert plan.sh_dim == (L + 1) ** 2
    assert [P.y_off for P in plan.paths_host] == [P.l2 ** 2 for P in plan.paths_host]
    # parity is free
    flipped = tuple((1, (l, 1)) for l in range(L + 1))
    assert equivariant.TPPlan(hid, flipped, o3.hidden_irreps(2, L)).sh_dim == (L + 1) ** 2
