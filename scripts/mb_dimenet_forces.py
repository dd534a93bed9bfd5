"""One measurement, no threshold: a DimeNet++ training step with and without a loss on the forces.

energy: E = model(batch); |E - y|.sum().backward()
forces: E, F = energy_and_forces(model, batch) (twice_differentiable=True, create_graph);
        (|E - y|.sum() + ((F - F*)^2).sum()).backward()

Default widths (hidden 128, int 64, basis (7, 6), basis_emb 8, four blocks) on the radius graph of
scripts/mb_dimenet.py (20000 nodes, mean degree 14: 263,600 edges, 3.54M triplets).  As there, the
two steps are timed alternately in one process with device events after three warm-up steps.
Prints one JSON line and, with --out, writes it to that file.

    python scripts/mb_dimenet_forces.py [--nodes 20000] [--degree 14] [--iters 5] [--windows 3]
                                        [--out profiles/dimenet_forces_mb.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "geometric-message-passing_amd"))
import gmp_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=20000)
ap.add_argument("--degree", type=float, default=14.0)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
r = 2.0
torch.manual_seed(0)
box = (args.nodes * 4.18879 * r ** 3 / args.degree) ** (1 / 3)
pos = torch.rand(args.nodes, 3, device=dev) * box
ei = gmp_amd.radius_graph_gpu(pos, r, max_num_neighbors=None)
atoms = torch.randint(1, 10, (args.nodes,), device=dev)
graph = torch.zeros(args.nodes, dtype=torch.long, device=dev)

model = gmp_amd.DimeNetPPModel(cutoff=2.5 * r, twice_differentiable=True).to(dev)
with torch.no_grad():  # PyG zero-initialises the last Linear of every output block
    for blk in model.output_blocks:
        blk.lin.weight.normal_(0.0, 0.05)
model.train()
y = torch.randn(1, 1, device=dev)
f_star = torch.randn(args.nodes, 3, device=dev)


def batch():
    return gmp_amd.Batch(atoms, pos.detach().clone(), ei, graph, num_graphs=1)


def energy_step():
    model.zero_grad(set_to_none=True)
    energy = model(batch())
    (energy - y).abs().sum().backward()
    return energy


def force_step():
    model.zero_grad(set_to_none=True)
    energy, forces = gmp_amd.energy_and_forces(model, batch())
    ((energy - y).abs().sum() + (forces - f_star).pow(2).sum()).backward()
    return forces


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for _ in range(3):
    energy_step(), force_step()
te, tf = [], []
for _ in range(max(3, args.windows)):  # alternate: other work shares the machine
    te.append(timed(energy_step, args.iters))
    tf.append(timed(force_step, args.iters))
with torch.no_grad():
    from gmp_amd.triplets import dimenet_triplets
    T = int(dimenet_triplets(ei, args.nodes)[-1].numel())
res = {"nodes": args.nodes, "edges": int(ei.shape[1]), "triplets": T,
       "energy_step_ms": [round(v, 3) for v in te], "force_step_ms": [round(v, 3) for v in tf],
       "ratio_of_medians": round(sorted(tf)[len(tf) // 2] / sorted(te)[len(te) // 2], 3)}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
