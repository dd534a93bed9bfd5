"""SphereNet on the host: the sympy-free basis tables, the module surface (state_dict, init,
errors) and the fp64 helper tests/spherenet_ref.py against the golden vectors of the reference
(tests/golden/spherenet.pt, made by tests/golden/make_golden_spherenet.py).  No GPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

import spherenet_ref as ref
from conftest import PKG, ROOT

CASES = ("A", "B", "C")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("spherenet.pt")


def _close(got, want, rel, what):
    scale = max(float(want.abs().max()), 1e-300) if want.numel() else 1.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= rel * scale, (what, err, scale)


def _ref_run(c):
    """The helper on a golden case: outputs, parameter gradients, geometry gradients."""
    g = c["geometry"]
    sd = {k: v.double().requires_grad_(True) for k, v in c["state_dict"].items()}
    geo = [g[k].double().requires_grad_(True) for k in ("dist", "angle", "torsion")]
    G = int(c["batch"].max()) + 1
    out = ref.model(sd, c["kwargs"], c["cutoff"], c["atoms"], geo[0], geo[1], geo[2], g["i"],
                    g["j"], g["idx_kj"], g["idx_ji"], c["batch"], G)
    (out * c["w"].double()).sum().backward()
    return out.detach(), sd, geo


@pytest.mark.parametrize("case", CASES)
def test_helper_reproduces_golden(gold, case):
    c = gold[case]
    g, kw, r64 = c["geometry"], c["kwargs"], c["ref64"]
    n, k = kw["num_spherical"], kw["num_radial"]
    rbf, a, t = ref.embeddings(g["dist"].double(), g["angle"].double(), g["torsion"].double(),
                               g["idx_kj"], c["state_dict"]["emb.dist_emb.freq"].double(), n, k,
                               c["cutoff"])
    rows = c["emb_rows"]
    _close(rbf, r64["dist_emb"], 1e-10, "dist_emb")
    _close(a[rows], r64["angle_emb"], 1e-10, "angle_emb")
    _close(t[rows], r64["torsion_emb"], 1e-10, "torsion_emb")
    out, sd, geo = _ref_run(c)
    _close(out, r64["out"], 1e-10, "out")
    for name, want in c["grads64"].items():
        _close(sd[name].grad, want, 1e-10, name)
    assert sorted(k for k, v in sd.items() if v.grad is None) == c["no_grad"]
    for t_, name in zip(geo, ("g_dist", "g_angle", "g_torsion")):
        _close(t_.grad, r64[name], 1e-10, name)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_matches_reference(gold, case):
    import gmp_amd
    c = gold[case]
    model = gmp_amd.SphereNetModel(cutoff=c["cutoff"], **c["kwargs"])
    sd = model.state_dict()
    assert list(sd) == list(c["state_dict"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == \
        {k: tuple(v.shape) for k, v in c["state_dict"].items()}
    model.load_state_dict(c["state_dict"], strict=True)
    for name in ("emb", "init", "update_e", "update_v", "ResidualLayer", "dist_emb"):
        assert isinstance(getattr(gmp_amd, name), type)
    tiny = dict(num_layers=1, hidden_channels=8, int_emb_size=4, out_emb_channels=8,
                num_spherical=2, num_radial=2)
    z = gmp_amd.SphereNetModel(output_init="zeros", **tiny)
    assert float(z.update_vs[0].lin.weight.detach().abs().max()) == 0.0
    assert float(gmp_amd.SphereNetModel(**tiny).update_vs[0].lin.weight.detach().abs().max()) > 0.0


def test_host_tables_small_x(gold):
    from gmp_amd.spherenet import basis_tables, sph_jl
    sx = gold["small_x"]
    zeros, norm, pref = basis_tables(7, 6)
    assert torch.equal(torch.from_numpy(zeros), sx["zeros"])
    assert torch.equal(torch.from_numpy(norm), sx["norm"])
    tab = sx["table"]
    # 1e-12 of each value (the smallest entry is ~1e-11, so a bound on the table's scale would
    # check nothing there).  At x = 1 the argument is the fp32-rounded zero itself and the value
    # is the residue of that rounding (~1e-8 N), ill-conditioned in the argument: there the
    # bound is 1e-12 of the function's scale N_lq.
    for xi, x in enumerate(sx["x"].tolist()):
        for l in range(7):
            for q in range(6):
                v = float(norm[l, q]) * sph_jl(l, float(zeros[l, q]) * x)
                want = float(tab[xi, l, q])
                scale = float(norm[l, q]) if x == 1.0 else abs(want)
                assert abs(v - want) <= 1e-12 * scale, (x, l, q, v, want)
    assert pref.shape == (49,) and abs(pref[0] - 0.28209479177387814) < 1e-15


def test_construction_is_quick_and_sympy_free():
    code = (
        "import sys, time\n"
        f"sys.path.insert(0, {PKG!r})\n"
        "import torch\n"
        "t = time.perf_counter()\n"
        "import gmp_amd\n"
        "m = gmp_amd.SphereNetModel()\n"
        "dt = time.perf_counter() - t\n"
        "bad = [k for k in ('sympy', 'scipy') if k in sys.modules]\n"
        "print('RESULT', dt, bad)\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][0]
    dt = float(line.split()[1])
    assert line.endswith("[]"), line
    assert dt < 5.0, dt


def test_glorot_orthogonal():
    from gmp_amd.spherenet import glorot_orthogonal
    torch.manual_seed(0)
    for shape in ((8, 42), (64, 8), (128, 128)):
        w = torch.empty(shape)
        glorot_orthogonal(w, scale=2.0)
        want_var = 2.0 / (shape[0] + shape[1])
        assert abs(float(w.var()) - want_var) <= 1e-5 * want_var
        g = w @ w.t() if shape[0] <= shape[1] else w.t() @ w
        d = torch.diagonal(g)
        assert float((g - torch.diag(d)).abs().max()) <= 1e-5 * float(d.max())
        assert float(d.max() - d.min()) <= 1e-4 * float(d.max())


def test_cpu_batch_raises(gold):
    import gmp_amd
    from gmp_amd import _lib
    from gmp_amd.graph import Batch
    c = gold["B"]
    model = gmp_amd.SphereNetModel(cutoff=c["cutoff"], **c["kwargs"])
    b = Batch(c["atoms"], c["pos"], c["edge_index"], c["batch"], num_graphs=2)
    with pytest.raises(_lib.GmpError):
        model(b)
    g = c["geometry"]
    with pytest.raises(_lib.GmpError):
        model.forward_from_geometry(c["atoms"], g["dist"], g["angle"], g["torsion"], g["i"],
                                    g["j"], g["idx_kj"], g["idx_ji"], c["batch"])
    b.edge_shift_idx = torch.zeros(c["edge_index"].shape[1], 3, dtype=torch.long)
    with pytest.raises(NotImplementedError):
        model(b)


def test_symbols_declared():
    from gmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "gmp.h")).read()
    names = ["gmp_sph_edge_basis_fwd_f32", "gmp_sph_edge_basis_bwd_f32",
             "gmp_sph_triplet_proj_fwd_f32", "gmp_sph_triplet_proj_bwd_f32",
             "gmp_sph_triplet_emb_f32", "gmp_triplet_interact_fwd_f32",
             "gmp_triplet_interact_bwd_f32"]
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 6
