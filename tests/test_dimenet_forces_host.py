"""The closed forms of tests/dimenet_bwd2_ref.py (what the *_bwd2 kernels of DimeNet++ evaluate)
against double autograd of tests/dimenet_ref.py, in fp64 on the CPU: both sides are fp64
evaluations of the same function, so each array agrees to 1e-10 of its scale.  Also the model's
twice_differentiable flag: off by default and absent from the state_dict."""
import pytest
import torch

import dimenet_bwd2_ref as ref2
import dimenet_ref as ref

TOL = 1e-10


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _check(name, got, want):
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    scale = _maxabs(want)
    err = _maxabs(got - want)
    print(f"{name}: err {err:.3e} scale {scale:.3e}")
    assert scale > 0, name
    assert err <= TOL * scale, (name, err, scale)


def _graph(N=14, r=2.2, seed=0):
    gen = torch.Generator().manual_seed(seed)
    pos = torch.rand(N, 3, generator=gen, dtype=torch.float64) * 3.0
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    src, dst = ((d < r) & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    return pos, torch.stack([src, dst]), gen


def _geometry(pos, ei, mode):
    """dimenet_ref.geometry (mode 1: the angle at vertex i); mode 0 moves the vertex to j."""
    dist, angle, i, j, idx_kj, idx_ji = ref.geometry(pos, ei)
    if mode == 0:
        row, col = ei
        jj, ii, kk = row[idx_ji], col[idx_ji], row[idx_kj]
        u, v = pos[ii] - pos[jj], pos[kk] - pos[jj]
        angle = torch.atan2(torch.linalg.cross(u, v).norm(dim=-1), (u * v).sum(-1))
    return dist, angle, idx_kj, idx_ji


@pytest.mark.parametrize("mode", [0, 1])
def test_geometry_bwd2(mode):
    pos, ei, gen = _graph()
    pos.requires_grad_(True)
    dist, angle, idx_kj, idx_ji = _geometry(pos, ei, mode)
    E, T = dist.numel(), angle.numel()
    assert E > 20 and T > 50
    assert float(torch.sin(angle.detach()).abs().min()) > 1e-3  # no collinear triplet
    g_dist = torch.randn(E, generator=gen, dtype=torch.float64).requires_grad_(True)
    g_angle = torch.randn(T, generator=gen, dtype=torch.float64).requires_grad_(True)
    a_pos = torch.randn(pos.shape, generator=gen, dtype=torch.float64)
    (g_pos,) = torch.autograd.grad((g_dist * dist).sum() + (g_angle * angle).sum(), pos,
                                   create_graph=True)
    want = torch.autograd.grad((a_pos * g_pos).sum(), (g_dist, g_angle, pos), retain_graph=True)
    got = ref2.geom_bwd2(pos.detach(), ei, idx_kj, idx_ji, mode, g_dist.detach(),
                         g_angle.detach(), a_pos)
    for name, g, w in zip(("gg_dist", "gg_angle", "h_pos"), got, want):
        _check(name, g, w)
    # an absent cotangent is a zero one
    only_d = ref2.geom_bwd2(pos.detach(), ei, idx_kj, idx_ji, mode, g_dist.detach(), None, a_pos)
    (g_pos,) = torch.autograd.grad((g_dist * dist).sum(), pos, create_graph=True)
    _check("h_pos (g_dist only)", only_d[2], torch.autograd.grad((a_pos * g_pos).sum(), pos)[0])


@pytest.mark.parametrize("exponent", [5, 1])
@pytest.mark.parametrize("nk", [(7, 6), (3, 2)])
def test_edge_basis_bwd2(nk, exponent):
    n, k = nk
    cutoff = 5.0
    gen = torch.Generator().manual_seed(1)
    E = 64
    x = 0.01 + 0.989 * torch.rand(E, generator=gen, dtype=torch.float64)
    x[0], x[1] = 0.01, 0.999
    dist = (x * cutoff).requires_grad_(True)
    freq = (torch.arange(1, k + 1, dtype=torch.float64) * torch.pi
            + 0.1 * torch.randn(k, generator=gen, dtype=torch.float64)).requires_grad_(True)

    def rnd(*sh):
        return torch.randn(*sh, generator=gen, dtype=torch.float64)

    g_rbf, g_sbe = rnd(E, k).requires_grad_(True), rnd(E, n * k).requires_grad_(True)
    a_dist, a_freq = rnd(E), rnd(k)
    rbf, sbe = ref.edge_basis(dist, freq, n, k, cutoff, exponent)
    gd, gf = torch.autograd.grad((g_rbf * rbf).sum() + (g_sbe * sbe).sum(), (dist, freq),
                                 create_graph=True)
    want = torch.autograd.grad((a_dist * gd).sum() + (a_freq * gf).sum(),
                               (g_rbf, g_sbe, dist, freq))
    got = ref2.edge_basis_bwd2(dist.detach(), freq.detach(), n, k, cutoff, exponent,
                               g_rbf.detach(), g_sbe.detach(), a_dist, a_freq)
    for name, g, w in zip(("gg_rbf", "gg_sbe", "h_dist", "h_freq"), got, want):
        _check(name, g, w)
    # beyond the cutoff: exact zeros
    far = torch.tensor([cutoff, 1.5 * cutoff], dtype=torch.float64)
    out = ref2.edge_basis_bwd2(far, freq.detach(), n, k, cutoff, exponent, rnd(2, k),
                               rnd(2, n * k), rnd(2), rnd(k))
    assert all(_maxabs(t) == 0.0 for t in out)


@pytest.mark.parametrize("nk", [(7, 6), (3, 2), (2, 6)])
def test_projection_bwd2(nk):
    n, k = nk
    L, b, E, T = 3, 5, 30, 97
    gen = torch.Generator().manual_seed(2)

    def rnd(*sh):
        return torch.randn(*sh, generator=gen, dtype=torch.float64)

    sbe = rnd(E, n * k).requires_grad_(True)
    angle = (0.02 + 3.1 * torch.rand(T, generator=gen, dtype=torch.float64)).requires_grad_(True)
    angle.data[0], angle.data[1] = 0.0, torch.pi  # the harmonics' derivatives are regular there
    idx_kj = torch.randint(0, E, (T,), generator=gen)
    W = rnd(L, b, n * k).requires_grad_(True)
    gS = rnd(L, T, b).requires_grad_(True)
    a_sbe, a_angle, a_W = rnd(E, n * k), rnd(T), rnd(L, b, n * k)
    sbf = ref.triplet_embedding(sbe, angle, idx_kj, n, k)
    S = torch.einsum("lbf,tf->ltb", W, sbf)
    gW, gsbe, gang = torch.autograd.grad((gS * S).sum(), (W, sbe, angle), create_graph=True)
    want = torch.autograd.grad((a_W * gW).sum() + (a_sbe * gsbe).sum() + (a_angle * gang).sum(),
                               (gS, W, sbe, angle))
    got = ref2.proj_bwd2(sbe.detach(), angle.detach(), idx_kj, n, k, W.detach(), gS.detach(),
                         a_sbe, a_angle, a_W)
    for name, g, w in zip(("gg_S", "h_W", "h_sbe", "h_angle"), got, want):
        _check(name, g, w)
    # each cotangent absent in turn equals a zero one
    for drop in range(3):
        a = [a_sbe, a_angle, a_W]
        a[drop] = None
        az = [torch.zeros_like(t) if i == drop else t for i, t in
              enumerate((a_sbe, a_angle, a_W))]
        for g, w in zip(ref2.proj_bwd2(sbe.detach(), angle.detach(), idx_kj, n, k, W.detach(),
                                       gS.detach(), *a),
                        ref2.proj_bwd2(sbe.detach(), angle.detach(), idx_kj, n, k, W.detach(),
                                       gS.detach(), *az)):
            assert torch.equal(g, w)


def test_bwd2_ops_registered_with_meta_kernels():
    """The two second-backward operators of TORCH_LIBRARY(gmp): shapes from the Meta kernels (no
    device work), absent cotangents accepted, and a CPU tensor refused at the boundary."""
    from gmp_amd import _lib
    tops = _lib.torch_ops()
    E, T, n, k, L, b = 11, 37, 7, 6, 3, 5
    m = dict(device="meta")
    dist, freq = torch.empty(E, **m), torch.empty(k, **m)
    zeros, norm = torch.empty(n, k, **m), torch.empty(n, k, **m)
    out = tops.dime_edge_basis_bwd2(dist, freq, zeros, norm, 5.0, 5, torch.empty(E, k, **m), None,
                                    torch.empty(E, **m), None)
    assert [tuple(t.shape) for t in out] == [(E, k), (E, n * k), (E,), (k,)]
    sbe, angle = torch.empty(E, n * k, **m), torch.empty(T, **m)
    idx, pref = torch.empty(T, dtype=torch.long, **m), torch.empty(n * n, **m)
    wt, gS = torch.empty(n * k, 16, **m), torch.empty(L, T, b, **m)
    for geom, Tg in ((True, T), (False, 0)):
        out = tops.dime_triplet_proj_bwd2(sbe, angle, idx, pref, wt, n, k, L, b, gS, None,
                                          torch.empty(T, **m), None, geom)
        assert [tuple(t.shape) for t in out] == [(L, T, b), (n * k, 16), (Tg, n * k), (Tg,)]
    with pytest.raises(RuntimeError, match="HIP device"):
        tops.dime_edge_basis_bwd2(torch.ones(2), torch.ones(k), torch.ones(n, k), torch.ones(n, k),
                                  5.0, 5, None, None, torch.ones(2), None)


def test_flag_is_not_state():
    import gmp_amd
    kw = dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16, num_layers=4)
    off = gmp_amd.DimeNetPPModel(**kw)
    on = gmp_amd.DimeNetPPModel(**kw, twice_differentiable=True)
    assert gmp_amd.DimeNetPPModel().twice_differentiable is False
    assert off.twice_differentiable is False and on.twice_differentiable is True
    assert list(off.state_dict()) == list(on.state_dict()) and len(off.state_dict()) == 147
    assert "twice_differentiable" not in dict(on.named_buffers())
    on.load_state_dict(off.state_dict(), strict=True)
    off.twice_differentiable = True  # a plain attribute: may be set after load_state_dict
    assert list(off.state_dict()) == list(on.state_dict())
    with pytest.raises(TypeError):
        gmp_amd.DimeNetPPModel(128, 1, 1, 4, 64, 8, 256, 7, 6, 10, 32, 5, 1, 2, 3, "swish", True)
