"""Two measurements, no threshold: SphereNet's periodic triplet geometry (K11p, edge-vector form).

(a) The geometry pass alone on the open radius graph of scripts/mb_dimenet.py (20000 nodes, mean
    degree 14: 263,600 edges, 3.54M triplets) with all shifts zero, vector form against K11's
    node form in the same run, each as the model runs it from pos to d pos:
      forward:  node  _run, mode 0 (count, fill with dist, angle, torsion and its winner)
                vec   edge_vectors (gather, subtract, add) + _run_dat_pbc (count, fill,
                      gmp_triplet_dat_pbc_f32)
      backward: node  gmp_triplet_geom_bwd_f32 + gmp_triplet_torsion_bwd_f32 + a CSR of
                      7T + 2E node ids + the segmented sum
                vec   gmp_triplet_dat_vec_bwd_f32 + two per-edge sums over cached CSRs +
                      EdgeVecToPosFn
(b) One inference energy_and_forces step of the default model on a periodic box (graph from
    radius_graph_pbc_gpu, periodic=True), alone and with stress=True, against the open-boundary
    step on a graph of the same density whose node count is chosen so that the edge counts match
    (the triplet counts follow; both are reported).

As in scripts/mb_dimenet_pbc.py: device events, three warm-up rounds, the variants alternating in
one process.  Prints one JSON line and, with --out, writes it to that file.

    python scripts/mb_spherenet_pbc.py [--nodes 20000] [--degree 14] [--iters 5] [--windows 3]
                                       [--out profiles/spherenet_pbc_mb.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "geometric-message-passing_amd"))
import gmp_amd  # noqa: E402
from gmp_amd import triplets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=20000)
ap.add_argument("--degree", type=float, default=14.0)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
r = 2.0
N = args.nodes
torch.manual_seed(0)
box = (N * 4.18879 * r ** 3 / args.degree) ** (1 / 3)
pos = torch.rand(N, 3, device=dev) * box
ei = gmp_amd.radius_graph_gpu(pos, r, max_num_neighbors=None)
E = int(ei.shape[1])


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns):
    """ms per call of each function: three warm-up rounds, then windows that alternate."""
    for _ in range(3):
        for f in fns.values():
            f()
    out = {k: [] for k in fns}
    for _ in range(max(3, args.windows)):
        for k, f in fns.items():
            out[k].append(round(timed(f, args.iters), 3))
    return out


# ------------------------------------------------------------------------------- (a) geometry
sidx = torch.zeros(E, 3, dtype=torch.int32, device=dev)
shift = torch.zeros(E, 3, device=dev)
p = pos.detach().clone().requires_grad_(True)
node_out = triplets.TripletGeomFn.apply(p, ei, N, 0, True)
vec_out = triplets.TripletVecDatFn.apply(triplets.edge_vectors(p, ei, shift), ei, N, sidx, True)
assert all(torch.equal(a, b) for a, b in zip(node_out, vec_out))  # bit for bit, lists included
T = int(node_out[3].numel())
cots = [torch.randn(E, device=dev), torch.randn(T, device=dev), torch.randn(T, device=dev)]


def backward(out):
    return lambda: torch.autograd.grad(out[:3], p, cots, retain_graph=True)


def no_grad(f):
    def run():
        with torch.no_grad():
            return f()
    return run


geom = alternate({
    "forward_node": no_grad(lambda: triplets._run(pos, ei, N, 0, True, True, True, True)),
    "forward_vec": no_grad(lambda: triplets._run_dat_pbc(
        triplets.edge_vectors(pos, ei, shift), ei, N, sidx, True)),
    "backward_node": backward(node_out),
    "backward_vec": backward(vec_out),
})
del node_out, vec_out

# ------------------------------------------------------------------------------- (b) inference
cell = torch.eye(3, device=dev) * box
ei_p, S_p = gmp_amd.radius_graph_pbc_gpu(pos, r, cell)
E_p = int(ei_p.shape[1])
n_open = int(round(N * E_p / E))  # same density, more nodes: the surface loses edges
pos_o = torch.rand(n_open, 3, device=dev) * box * (n_open / N) ** (1 / 3)
ei_o = gmp_amd.radius_graph_gpu(pos_o, r, max_num_neighbors=None)
with torch.no_grad():
    T_p = int(triplets.dimenet_triplets(ei_p, N, S_p)[-1].numel())
    T_o = int(triplets.dimenet_triplets(ei_o, n_open)[-1].numel())

model = gmp_amd.SphereNetModel(cutoff=2.5 * r, periodic=True).to(dev).eval()
n_max = max(N, n_open)
atoms = torch.randint(1, 10, (n_max,), device=dev)
zeros = torch.zeros(n_max, dtype=torch.long, device=dev)
edge_graph = torch.zeros(E_p, dtype=torch.long, device=dev)


def periodic_batch():
    return gmp_amd.Batch(atoms[:N], pos.detach().clone(), ei_p, zeros[:N], num_graphs=1,
                         cell=cell.view(1, 3, 3), pbc=(True, True, True), edge_shift_idx=S_p,
                         edge_graph=edge_graph)


def open_step():
    b = gmp_amd.Batch(atoms[:n_open], pos_o.detach().clone(), ei_o, zeros[:n_open], num_graphs=1)
    return gmp_amd.energy_and_forces(model, b)


step = alternate({
    "open": open_step,
    "periodic": lambda: gmp_amd.energy_and_forces(model, periodic_batch()),
    "periodic_with_stress": lambda: gmp_amd.energy_and_forces(model, periodic_batch(),
                                                              stress=True),
})


def med(v):
    return sorted(v)[len(v) // 2]


res = {
    "geometry": {"nodes": N, "edges": E, "triplets": T, "ms": geom,
                 "vec_over_node_medians": {
                     k: round(med(geom[k + "_vec"]) / med(geom[k + "_node"]), 3)
                     for k in ("forward", "backward")}},
    "inference_step": {"periodic": {"nodes": N, "edges": E_p, "triplets": T_p},
                       "open": {"nodes": n_open, "edges": int(ei_o.shape[1]), "triplets": T_o},
                       "ms": step,
                       "periodic_with_stress_over_open_medians": round(
                           med(step["periodic_with_stress"]) / med(step["open"]), 3)},
}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
