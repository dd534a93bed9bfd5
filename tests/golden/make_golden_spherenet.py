"""Golden vectors for SphereNet from the reference's own code (tests/golden/spherenet.pt).

Run once in the development container (needs the reference checkout, sympy and scipy; about
four minutes, nearly all of it the reference's sympy basis construction):

    python tests/golden/make_golden_spherenet.py [/path/to/reference]

models/layers/spherenet_layer.py and models/spherenet.py are loaded through _ref_stubs.  The
geometry (dist, angle, torsion, index lists) is computed once by the reference's fp32
xyz_to_dat and then held fixed: the module's xyz_to_dat is replaced by a function returning it,
as fp32 leaves for the fp32 run and upcast for the .double() run.  (The torsion is a scatter-min
over candidates of which one is rounding residue, so fp32 and fp64 geometry disagree on the
winner; everything downstream is compared on the same geometry.)

Per case: the inputs, the state_dict, and from the fp64 run the outputs, all parameter
gradients of (out * w).sum(), the geometry gradients, the names of the parameters without a
gradient, and the three embeddings (dist_emb in full, angle_emb / torsion_emb on the rows
`emb_rows`: the full torsion_emb of case C alone would be 11 MB); plus the fp32 reference's own
error against fp64 for each (err32).  All edge lengths keep d / cutoff >= 0.2, where the
reference's closed-form Bessel functions are trustworthy in fp64; the generator asserts
err32 <= 1e-4 max(1, scale) for outputs and parameter gradients.

A rerun reproduces every stored tensor bit for bit.  The err32 figures come from the fp32 run,
whose CPU scatter-adds depend on the thread schedule: one of them moved in its second digit
between two runs (2.20e-5 -> 2.30e-5).

Also the small-x table: N_lq j_l(z_lq x) for (7, 6) from scipy's spherical_jn in fp64, with the
reference's zeros and normalisers (stored too).
"""
import copy
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

np.math = math  # the reference calls np.math.factorial (gone in numpy 2)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
CUTOFF = 5.0


def load():
    mods = _ref_stubs.load_reference(REF)
    name = "models.spherenet"
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "models/spherenet.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mods["models.layers.spherenet_layer"], mod


def scattered(n, gen, lo=1.0, box=3.2):
    """n points with all pair distances >= lo, by rejection."""
    pts = []
    while len(pts) < n:
        p = (torch.rand(3, generator=gen) * box)
        if all((p - q).norm() >= lo for q in pts):
            pts.append(p)
    return torch.stack(pts)


def radius_edges(pos, batch, r):
    d = (pos[:, None] - pos[None]).norm(dim=-1)
    m = (d < r) & (batch[:, None] == batch[None]) & ~torch.eye(len(pos), dtype=torch.bool)
    src, dst = m.nonzero(as_tuple=True)
    return torch.stack([src, dst])


def molecule_graph(sizes, seed, r=2.0):
    """Graphs of the given sizes; the last node of the last graph is a pendant (one neighbour),
    so its outgoing edge owns no triplet."""
    gen = torch.Generator().manual_seed(seed)
    pos, batch = [], []
    for g, n in enumerate(sizes):
        p = scattered(n, gen)
        if g == len(sizes) - 1:
            # 1.9 above the topmost node: every other node is then at least sqrt(4.61) > r away
            p[-1] = p[p[:-1, 2].argmax()] + torch.tensor([0.0, 0.0, 1.9])
        pos.append(p + 10.0 * g)
        batch += [g] * n
    pos, batch = torch.cat(pos), torch.tensor(batch)
    return pos, batch, radius_edges(pos, batch, r)


def hub_graph(leaves=70, radius=2.4):
    i = torch.arange(leaves, dtype=torch.float64) + 0.5
    phi = torch.acos(1 - 2 * i / leaves)
    th = math.pi * (1 + 5 ** 0.5) * i
    pts = radius * torch.stack([torch.cos(th) * torch.sin(phi), torch.sin(th) * torch.sin(phi),
                                torch.cos(phi)], 1)
    pos = torch.cat([torch.zeros(1, 3, dtype=torch.float64), pts]).float()
    leaf = torch.arange(1, leaves + 1)
    hub = torch.zeros(leaves, dtype=torch.long)
    ei = torch.cat([torch.stack([hub, leaf]), torch.stack([leaf, hub])], 1)
    return pos, torch.zeros(leaves + 1, dtype=torch.long), ei


def randomise(model, gen):
    for name, p in model.named_parameters():
        if name.endswith("freq"):
            continue
        fan_in = p.shape[1] if p.dim() == 2 and "emb.weight" not in name else 1
        if name.endswith("bias"):
            fan_in = dict(model.named_parameters())[name[:-4] + "weight"].shape[1]
        p.data = torch.randn(p.shape, generator=gen) / math.sqrt(fan_in)


def run(sn, model, geom, atoms, pos, ei, batch, w, dtype):
    dist, angle, torsion, i, j, idx_kj, idx_ji = geom
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (dist, angle, torsion)]
    sn.xyz_to_dat = lambda *a, **k: (leaves[0], leaves[1], leaves[2], i, j, idx_kj, idx_ji)
    data = types.SimpleNamespace(atoms=atoms, pos=pos.to(dtype), edge_index=ei, batch=batch)
    model.zero_grad(set_to_none=True)
    out = model(data)
    (out * w.to(dtype)).sum().backward()
    with torch.no_grad():
        embs = model.emb(leaves[0], leaves[1], leaves[2], idx_kj)
    res = {"out": out.detach(), "g_dist": leaves[0].grad, "g_angle": leaves[1].grad,
           "g_torsion": leaves[2].grad, "dist_emb": embs[0], "angle_emb": embs[1],
           "torsion_emb": embs[2]}
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None}
    nograd = sorted(n for n, p in model.named_parameters() if p.grad is None)
    return res, grads, nograd


def make_case(layer, sn, name, graph, seed, zero_segments=True, **kw):
    pos, batch, ei = graph
    gen = torch.Generator().manual_seed(seed)
    atoms = torch.randint(1, 10, (pos.shape[0],), generator=gen)
    model = sn.SphereNetModel(cutoff=CUTOFF, **kw)
    randomise(model, gen)
    with torch.no_grad():
        geom = layer.xyz_to_dat(pos, ei, pos.shape[0], use_torsion=True)
    dist, angle, torsion, i, j, idx_kj, idx_ji = geom
    assert bool((idx_ji[1:] >= idx_ji[:-1]).all())
    assert float(dist.min()) / CUTOFF >= 0.2, float(dist.min())
    counts = torch.bincount(idx_ji, minlength=dist.numel())
    if zero_segments:
        assert int(counts.min()) == 0, "the case must hold edges without triplets"
    G, od = int(batch.max()) + 1, kw["out_dim"]
    w = 1.0 + 0.37 * torch.arange(G).view(-1, 1) - 0.21 * torch.arange(od).view(1, -1)
    r32, g32, ng32 = run(sn, model, geom, atoms, pos, ei, batch, w, torch.float32)
    m64 = copy.deepcopy(model).double()
    r64, g64, ng64 = run(sn, m64, geom, atoms, pos, ei, batch, w, torch.float64)
    assert ng32 == ng64
    T = angle.numel()
    rows = torch.arange(0, T, max(1, T // 32))[:32]
    err32 = {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}
    r64["angle_emb"], r64["torsion_emb"] = r64["angle_emb"][rows], r64["torsion_emb"][rows]
    err32["grads"] = {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}
    scale = max(1.0, float(r64["out"].abs().max()))
    assert err32["out"] <= 1e-4 * scale, (name, err32["out"], scale)
    for k, g in g64.items():
        assert err32["grads"][k] <= 1e-4 * max(1.0, float(g.abs().max())), (name, k)
    print(f"case {name}: N {pos.shape[0]} E {dist.numel()} T {T} (per edge {int(counts.min())}.."
          f"{int(counts.max())}), min d/cutoff {float(dist.min()) / CUTOFF:.3f}, |out| "
          f"{scale:.3g}, err32 out {err32['out']:.2e}, worst grad "
          f"{max(err32['grads'].values()):.2e}, {len(ng64)} parameters without gradient")
    return {"kwargs": {k: v for k, v in kw.items()}, "cutoff": CUTOFF, "atoms": atoms, "pos": pos,
            "edge_index": ei, "batch": batch, "w": w,
            "geometry": {"dist": dist, "angle": angle, "torsion": torsion, "i": i, "j": j,
                         "idx_kj": idx_kj, "idx_ji": idx_ji},
            "state_dict": {k: v.clone() for k, v in model.state_dict().items()},
            "emb_rows": rows, "ref64": r64, "grads64": g64, "no_grad": ng64, "err32": err32}


def small_x_table(layer, n=7, k=6):
    from scipy.special import spherical_jn
    zeros = layer.Jn_zeros(n, k)
    norm = np.stack([1 / np.array([0.5 * layer.Jn(zeros[l, q], l + 1) ** 2
                                   for q in range(k)]) ** 0.5 for l in range(n)])
    xs = np.array([0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0])
    tab = np.zeros((len(xs), n, k))
    for l in range(n):
        for q in range(k):
            tab[:, l, q] = float(norm[l, q]) * spherical_jn(l, float(zeros[l, q]) * xs)
    return {"x": torch.from_numpy(xs), "table": torch.from_numpy(tab),
            "zeros": torch.from_numpy(zeros.astype(np.float32)),
            "norm": torch.from_numpy(norm.astype(np.float32)),
            "norm_dtype": str(norm.dtype)}


def main():
    torch.manual_seed(0)
    layer, sn = load()
    out = {"small_x": small_x_table(layer)}
    small = dict(num_spherical=7, num_radial=6, basis_emb_size_dist=8, basis_emb_size_angle=8,
                 basis_emb_size_torsion=8, hidden_channels=16, int_emb_size=8,
                 out_emb_channels=16, out_dim=2)
    out["A"] = make_case(layer, sn, "A", molecule_graph([8, 6], 11), 1, num_layers=2, **small)
    out["B"] = make_case(layer, sn, "B", molecule_graph([7, 5], 12), 2, num_layers=2,
                         num_spherical=3, num_radial=2, basis_emb_size_dist=5,
                         basis_emb_size_angle=3, basis_emb_size_torsion=4, hidden_channels=12,
                         int_emb_size=6, out_emb_channels=16, out_dim=2,
                         use_node_features=False)
    out["C"] = make_case(layer, sn, "C", hub_graph(), 3, num_layers=1, **small)
    path = os.path.join(HERE, "spherenet.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
