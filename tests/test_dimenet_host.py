"""DimeNet++ on the host: the fp64 helper tests/dimenet_ref.py against the golden basis vectors of
the reference (tests/golden/spherenet.pt: SphereNet's angle_emb is DimeNet's spherical basis
without the envelope), the module surface (state_dict keys and shapes, initialisation), the Meta
kernels of the new operators, and the helper's own invariances.  No GPU."""
import math
import os
import re

import pytest
import torch

import dimenet_ref as ref
import spherenet_ref as sref
from conftest import ROOT

CASES = ("A", "B", "C")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("spherenet.pt")


def _close(got, want, rel, what):
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= rel * scale, (what, err, scale)


# ----------------------------------------------------------------------------------- 1. basis
@pytest.mark.parametrize("case", CASES)
def test_basis_against_golden(gold, case):
    c = gold[case]
    g, kw, r64 = c["geometry"], c["kwargs"], c["ref64"]
    n, k, cutoff = kw["num_spherical"], kw["num_radial"], c["cutoff"]
    dist, angle, idx_kj = g["dist"].double(), g["angle"].double(), g["idx_kj"]
    freq = c["state_dict"]["emb.dist_emb.freq"].double()
    rbf, sbf = ref.bases(dist, angle, idx_kj, freq, n, k, cutoff)
    rows = c["emb_rows"]
    x = dist / cutoff
    mask = (x < 1.0).double()
    env = sref.envelope(x, 5) * mask
    _close(sbf[rows], env[idx_kj][rows].unsqueeze(-1) * r64["angle_emb"], 1e-10, "sbf")
    _close(rbf, mask.unsqueeze(-1) * r64["dist_emb"], 1e-10, "rbf")
    assert float(sbf.abs().max()) > 0 and float(rbf.abs().max()) > 0


# ----------------------------------------------------------------------------------- 2. keys
def _expected_keys(H=128, I=64, b=8, O=256, n=7, k=6, out_dim=1, L=4, before=1, after=2, lins=3):
    keys = [("rbf.freq", (k,)),
            ("emb.emb.weight", (95, H)),
            ("emb.lin_rbf.weight", (H, k)), ("emb.lin_rbf.bias", (H,)),
            ("emb.lin.weight", (H, 3 * H)), ("emb.lin.bias", (H,))]
    for l in range(L + 1):
        p = f"output_blocks.{l}."
        keys += [(p + "lin_rbf.weight", (H, k)), (p + "lin_up.weight", (O, H))]
        for m in range(lins):
            keys += [(p + f"lins.{m}.weight", (O, O)), (p + f"lins.{m}.bias", (O,))]
        keys += [(p + "lin.weight", (out_dim, O))]

    def res(p):
        return [(p + "lin1.weight", (H, H)), (p + "lin1.bias", (H,)),
                (p + "lin2.weight", (H, H)), (p + "lin2.bias", (H,))]

    for l in range(L):
        p = f"interaction_blocks.{l}."
        keys += [(p + "lin_rbf1.weight", (b, k)), (p + "lin_rbf2.weight", (H, b)),
                 (p + "lin_sbf1.weight", (b, n * k)), (p + "lin_sbf2.weight", (I, b)),
                 (p + "lin_kj.weight", (H, H)), (p + "lin_kj.bias", (H,)),
                 (p + "lin_ji.weight", (H, H)), (p + "lin_ji.bias", (H,)),
                 (p + "lin_down.weight", (I, H)), (p + "lin_up.weight", (H, I))]
        for m in range(before):
            keys += res(p + f"layers_before_skip.{m}.")
        keys += [(p + "lin.weight", (H, H)), (p + "lin.bias", (H,))]
        for m in range(after):
            keys += res(p + f"layers_after_skip.{m}.")
    return keys


def test_keys_and_shapes():
    import gmp_amd
    torch.manual_seed(0)
    model = gmp_amd.DimeNetPPModel()
    sd = model.state_dict()
    want = _expected_keys()
    assert len(want) == 147 == 1 + 5 + 5 * 9 + 4 * 24
    assert [(key, tuple(v.shape)) for key, v in sd.items()] == want
    assert sorted(name for name, _ in model.named_parameters()) == sorted(key for key, _ in want)
    # the basis tables are buffers, but not persistent ones
    assert sorted(name for name, _ in model.named_buffers()) == ["sbf.norm", "sbf.pref",
                                                                 "sbf.zeros"]
    for l in range(5):
        assert float(sd[f"output_blocks.{l}.lin.weight"].abs().max()) == 0.0
    assert torch.equal(sd["rbf.freq"], torch.arange(1, 7).float() * math.pi)
    for key in ("interaction_blocks.0.lin_kj.bias", "output_blocks.1.lins.0.bias",
                "interaction_blocks.3.layers_after_skip.1.lin2.bias"):
        assert float(sd[key].abs().max()) == 0.0
    w = sd["interaction_blocks.2.lin_down.weight"]  # glorot_orthogonal(scale=2)
    assert abs(float(w.var()) - 2.0 / (64 + 128)) <= 1e-5 * 2.0 / (64 + 128)
    assert float(sd["emb.emb.weight"].abs().max()) <= math.sqrt(3)
    # round trip, strict
    gen = torch.Generator().manual_seed(1)
    sd2 = {key: torch.randn(v.shape, generator=gen) for key, v in sd.items()}
    other = gmp_amd.DimeNetPPModel()
    other.load_state_dict(sd2, strict=True)
    back = other.state_dict()
    assert list(back) == list(sd2) and all(torch.equal(back[key], sd2[key]) for key in sd2)
    # other widths, a callable activation, the unused arguments
    small = gmp_amd.DimeNetPPModel(hidden_channels=16, in_dim=3, out_dim=2, num_layers=2,
                                   int_emb_size=8, basis_emb_size=4, out_emb_channels=32,
                                   num_spherical=3, num_radial=2, max_num_neighbors=5,
                                   num_before_skip=2, num_after_skip=1, num_output_layers=1,
                                   act=torch.tanh)
    assert [(key, tuple(v.shape)) for key, v in small.state_dict().items()] == \
        _expected_keys(H=16, I=8, b=4, O=32, n=3, k=2, out_dim=2, L=2, before=2, after=1, lins=1)
    with pytest.raises(ValueError):
        gmp_amd.DimeNetPPModel(act="relu6")
    assert "DimeNetPPModel" in gmp_amd.__all__


def test_symbols_declared():
    from gmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmp.h")).read()
    names = ["gmp_dime_edge_basis_fwd_f32", "gmp_dime_edge_basis_bwd_f32",
             "gmp_dime_edge_basis_bwd_partial_rows", "gmp_dime_triplet_proj_fwd_f32",
             "gmp_dime_triplet_proj_bwd_f32", "gmp_dime_triplet_proj_bwd_partial_rows",
             "gmp_dime_triplet_emb_f32", "gmp_triplet_interact1_fwd_f32",
             "gmp_triplet_interact1_bwd_f32", "gmp_triplet_interact1_bwd_partial_rows"]
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 6
    assert re.search(r"#define\s+GMP_ABI_VERSION\s+6\b", header)


# ----------------------------------------------------------------------------------- 3. Meta
def test_meta_shapes_and_cpu_tensors_rejected():
    from gmp_amd import _lib
    tops = _lib.torch_ops()
    for name in ("dime_edge_basis_fwd", "dime_edge_basis_bwd", "dime_triplet_proj_fwd",
                 "dime_triplet_proj_bwd", "dime_triplet_emb", "triplet_interact1_fwd",
                 "triplet_interact1_bwd"):
        assert hasattr(tops, name), name
    E, T, n, k, L, b, I = 700, 5000, 7, 6, 4, 8, 64
    f = dict(device="meta")
    i64 = dict(dtype=torch.long, device="meta")
    dist, freq = torch.empty(E, **f), torch.empty(k, **f)
    zeros, norm, pref = torch.empty(n, k, **f), torch.empty(n, k, **f), torch.empty(n * n, **f)
    rbf, sbe = tops.dime_edge_basis_fwd(dist, freq, zeros, norm, 5.0, 5)
    assert tuple(rbf.shape) == (E, k) and tuple(sbe.shape) == (E, n * k)
    gd, gf = tops.dime_edge_basis_bwd(dist, freq, zeros, norm, 5.0, 5, rbf, None)
    assert tuple(gd.shape) == (E,) and tuple(gf.shape) == (k,)
    angle, idx = torch.empty(T, **f), torch.empty(T, **i64)
    wt = torch.empty(n * k, L * b, **f)
    S = tops.dime_triplet_proj_fwd(sbe, angle, idx, pref, wt, n, k, L, b)
    assert tuple(S.shape) == (L, T, b)
    assert tuple(tops.dime_triplet_emb(sbe, angle, idx, pref, n, k).shape) == (T, n * k)
    gw, gs, ga = tops.dime_triplet_proj_bwd(sbe, angle, idx, pref, wt, n, k, L, b, S, True)
    assert tuple(gw.shape) == (n * k, L * b) and tuple(gs.shape) == (T, n * k)
    assert tuple(ga.shape) == (T,)
    gw, gs, ga = tops.dime_triplet_proj_bwd(sbe, angle, idx, pref, wt, n, k, L, b, S, False)
    assert tuple(gs.shape) == (0, n * k) and tuple(ga.shape) == (0,)
    xd, W = torch.empty(E, I, **f), torch.empty(I, b, **f)
    m = tops.triplet_interact1_fwd(xd, S[0], W, idx, None, torch.empty(E + 1, **i64))
    assert tuple(m.shape) == (E, I)
    m = tops.triplet_interact1_fwd(xd, S[0], W, idx, idx, torch.empty(301, **i64))
    assert tuple(m.shape) == (300, I)
    gS, gW = tops.triplet_interact1_bwd(m.new_empty(E, I), xd, S[0], W, idx,
                                        torch.empty(E + 1, **i64))
    assert tuple(gS.shape) == (T, b) and tuple(gW.shape) == (I, b)
    # CPU tensors: the boundary's error, never a fallback
    with pytest.raises(RuntimeError, match="HIP device"):
        tops.dime_edge_basis_fwd(torch.ones(3), torch.ones(6), torch.ones(7, 6),
                                 torch.ones(7, 6), 5.0, 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        tops.triplet_interact1_fwd(torch.ones(2, 4), torch.ones(0, 8), torch.ones(4, 8),
                                   torch.zeros(0, dtype=torch.long), None,
                                   torch.zeros(3, dtype=torch.long))


def test_cpu_batch_raises():
    import gmp_amd
    from gmp_amd import _lib
    from gmp_amd.graph import Batch
    model = gmp_amd.DimeNetPPModel(hidden_channels=16, int_emb_size=8, out_emb_channels=16,
                                   num_layers=1)
    pos = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    ei = torch.tensor([[0, 1, 1, 2, 0, 2], [1, 0, 2, 1, 2, 0]])
    b = Batch(torch.ones(3, dtype=torch.long), pos, ei, torch.zeros(3, dtype=torch.long),
              num_graphs=1)
    with pytest.raises(_lib.GmpError):
        model(b)
    b.edge_shift_idx = torch.zeros(6, 3, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        model(b)


# ----------------------------------------------------------------------------------- 4. helper
def _helper_case(seed=0, N=14):
    import gmp_amd
    gen = torch.Generator().manual_seed(seed)
    pts = torch.zeros(0, 3, dtype=torch.float64)
    while pts.shape[0] < N:
        p = torch.rand(1, 3, generator=gen, dtype=torch.float64) * 2.8
        if pts.shape[0] == 0 or float((pts - p).norm(dim=1).min()) >= 1.0:
            pts = torch.cat([pts, p])
    batch = (torch.arange(N) >= N // 2).long()
    d = (pts[:, None] - pts[None]).norm(dim=-1)
    same = batch[:, None] == batch[None]
    src, dst = ((d < 2.0) & same & ~torch.eye(N, dtype=torch.bool)).nonzero(as_tuple=True)
    atoms = torch.randint(1, 10, (N,), generator=gen)
    kw = dict(hidden_channels=16, int_emb_size=8, out_emb_channels=16, num_layers=2, cutoff=1.8)
    torch.manual_seed(seed)
    model = gmp_amd.DimeNetPPModel(**kw)
    sd = {key: v.double() for key, v in model.state_dict().items()}
    for l in range(3):  # PyG's zero initialisation would make the output identically zero
        key = f"output_blocks.{l}.lin.weight"
        sd[key] = torch.randn(sd[key].shape, generator=gen, dtype=torch.float64)
    return sd, kw, atoms, pts, torch.stack([src, dst]), batch


def _helper_energy(sd, kw, atoms, pos, ei, batch):
    dist, angle, i, j, idx_kj, idx_ji = ref.geometry(pos, ei)
    return ref.model(sd, kw, atoms, dist, angle, i, j, idx_kj, idx_ji, batch, 2), dist


def test_helper_invariance_and_forces():
    sd, kw, atoms, pts, ei, batch = _helper_case()
    pos = pts.clone().requires_grad_(True)
    out, dist = _helper_energy(sd, kw, atoms, pos, ei, batch)
    assert tuple(out.shape) == (2, 1) and float(out.detach().abs().max()) > 0
    # both sides of the cutoff (1.8) are present, so the [x < 1] factor takes part
    assert bool((dist < 1.8).any()) and bool((dist >= 1.8).any())
    (g,) = torch.autograd.grad(out.sum(), pos)
    F = -g
    assert float(F.abs().max()) > 0
    assert float(F.sum(0).abs().max()) <= 1e-10 * max(1.0, float(F.abs().max()))
    gen = torch.Generator().manual_seed(5)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
    shift = torch.randn(1, 3, generator=gen, dtype=torch.float64)
    out2, _ = _helper_energy(sd, kw, atoms, pts @ Q.t() + shift, ei, batch)
    scale = max(1.0, float(out.detach().abs().max()))
    assert float((out2 - out.detach()).abs().max()) <= 1e-10 * scale
