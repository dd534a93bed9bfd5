"""Two measurements, no threshold: DimeNet++'s periodic triplet geometry (K11p, edge-vector form).

(a) The geometry pass alone on the open radius graph of scripts/mb_dimenet.py (20000 nodes, mean
    degree 14: 263,600 edges, 3.54M triplets) with all shifts zero, vector form against the
    existing node form, each as the model runs it from pos to d pos:
      fill:  node  _run (count, fill with dist and angle)
             vec   edge_vectors (gather, subtract, add) + _run_pbc
      bwd:   node  gmp_triplet_geom_bwd_f32 + a CSR of 3T + 2E node ids + the segmented sum
             vec   gmp_triplet_vec_bwd_f32 + two per-edge sums over cached CSRs + EdgeVecToPosFn
      bwd2:  the second backward of the same, to (g_dist, g_angle, pos)
(b) One force-training step (|E - y| + (F - F*)^2) at default widths on a periodic box (graph
    from radius_graph_pbc_gpu, periodic=True), alone and with the stress term, against the
    open-boundary step on a graph of the same density whose node count is chosen so that the
    edge counts match (the triplet counts follow; both are reported).

As in scripts/mb_dimenet_forces.py: device events, three warm-up steps, the variants alternating
in one process.  Prints one JSON line and, with --out, writes it to that file.

    python scripts/mb_dimenet_pbc.py [--nodes 20000] [--degree 14] [--iters 5] [--windows 3]
                                     [--out profiles/dimenet_pbc_mb.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "geometric-message-passing_amd"))
import gmp_amd  # noqa: E402
from gmp_amd import ops, triplets  # noqa: E402

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
    """Median ms per call of each function: three warm-up rounds, then windows that alternate."""
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
with torch.no_grad():
    _, _, _, idx_kj, idx_ji = triplets._run(pos, ei, N, 1, True, False, True)
    vec0 = triplets.edge_vectors(pos, ei, shift)
    lists = triplets._run_pbc(vec0, ei, N, sidx)
    assert torch.equal(lists[2], idx_kj) and torch.equal(lists[3], idx_ji)
T = int(idx_kj.numel())
g_dist = torch.randn(E, device=dev).requires_grad_(True)
g_angle = torch.randn(T, device=dev).requires_grad_(True)
a_pos = torch.randn(N, 3, device=dev)
p = pos.detach().clone().requires_grad_(True)


def node_bwd():
    return triplets.TripletGeomBwdFn.apply(p, ei, idx_kj, idx_ji, g_dist, g_angle, 1, N)


def vec_bwd():
    vec = triplets.edge_vectors(p, ei, shift)
    g_vec = triplets.TripletVecGeomBwdFn.apply(vec, idx_kj, idx_ji, g_dist, g_angle)
    return ops.EdgeVecToPosFn.apply(g_vec, ei, N)


def second(first):
    return torch.autograd.grad((first() * a_pos).sum(), (g_dist, g_angle, p))


def no_grad(f):
    def run():
        with torch.no_grad():
            return f()
    return run


geom = alternate({
    "fill_node": no_grad(lambda: triplets._run(pos, ei, N, 1, True, False, True)),
    "fill_vec": no_grad(lambda: triplets._run_pbc(triplets.edge_vectors(pos, ei, shift), ei, N,
                                                  sidx)),
    "bwd_node": no_grad(node_bwd),
    "bwd_vec": no_grad(vec_bwd),
    "bwd_plus_bwd2_node": lambda: second(node_bwd),
    "bwd_plus_bwd2_vec": lambda: second(vec_bwd),
})

# ------------------------------------------------------------------------------- (b) the step
cell = torch.eye(3, device=dev) * box
ei_p, S_p = gmp_amd.radius_graph_pbc_gpu(pos, r, cell)
E_p = int(ei_p.shape[1])
n_open = int(round(N * E_p / E))  # same density, more nodes: the surface loses edges
pos_o = torch.rand(n_open, 3, device=dev) * box * (n_open / N) ** (1 / 3)
ei_o = gmp_amd.radius_graph_gpu(pos_o, r, max_num_neighbors=None)
with torch.no_grad():
    T_p = int(triplets.dimenet_triplets(ei_p, N, S_p)[-1].numel())
    T_o = int(triplets.dimenet_triplets(ei_o, n_open)[-1].numel())

model = gmp_amd.DimeNetPPModel(cutoff=2.5 * r, twice_differentiable=True, periodic=True).to(dev)
with torch.no_grad():  # PyG zero-initialises the last Linear of every output block
    for blk in model.output_blocks:
        blk.lin.weight.normal_(0.0, 0.05)
model.train()
y = torch.randn(1, 1, device=dev)
n_max = max(N, n_open)
atoms = torch.randint(1, 10, (n_max,), device=dev)
f_star = torch.randn(n_max, 3, device=dev)
s_star = torch.randn(1, 3, 3, device=dev) * 0.01
zeros = torch.zeros(n_max, dtype=torch.long, device=dev)
edge_graph = torch.zeros(E_p, dtype=torch.long, device=dev)


def periodic_batch():
    return gmp_amd.Batch(atoms[:N], pos.detach().clone(), ei_p, zeros[:N], num_graphs=1,
                         cell=cell.view(1, 3, 3), pbc=(True, True, True), edge_shift_idx=S_p,
                         edge_graph=edge_graph)


def open_step():
    model.zero_grad(set_to_none=True)
    b = gmp_amd.Batch(atoms[:n_open], pos_o.detach().clone(), ei_o, zeros[:n_open], num_graphs=1)
    energy, forces = gmp_amd.energy_and_forces(model, b)
    ((energy - y).abs().sum() + (forces - f_star[:n_open]).pow(2).sum()).backward()


def periodic_step():
    model.zero_grad(set_to_none=True)
    energy, forces = gmp_amd.energy_and_forces(model, periodic_batch())
    ((energy - y).abs().sum() + (forces - f_star[:N]).pow(2).sum()).backward()


def periodic_stress_step():
    model.zero_grad(set_to_none=True)
    energy, forces, sigma = gmp_amd.energy_and_forces(model, periodic_batch(), stress=True)
    ((energy - y).abs().sum() + (forces - f_star[:N]).pow(2).sum()
     + (sigma - s_star).pow(2).sum()).backward()


step = alternate({"open": open_step, "periodic": periodic_step,
                  "periodic_with_stress": periodic_stress_step})


def med(v):
    return sorted(v)[len(v) // 2]


res = {
    "geometry": {"nodes": N, "edges": E, "triplets": T, "ms": geom,
                 "vec_over_node_medians": {
                     k: round(med(geom[k + "_vec"]) / med(geom[k + "_node"]), 3)
                     for k in ("fill", "bwd", "bwd_plus_bwd2")}},
    "force_step": {"periodic": {"nodes": N, "edges": E_p, "triplets": T_p},
                   "open": {"nodes": n_open, "edges": int(ei_o.shape[1]), "triplets": T_o},
                   "ms": step,
                   "periodic_over_open_medians": round(med(step["periodic"]) / med(step["open"]),
                                                       3)},
}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
