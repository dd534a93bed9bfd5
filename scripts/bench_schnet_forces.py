"""Timing record of an energy-and-force training step for SchNet (stand-alone; bench.py is
untouched).

Workload: the bench graph radius_graph(50_000, 1_000_000), SchNetModel at its defaults.  A force
step is forward, force gradient with create_graph, the combined loss sum |E - y| + sum (F - F*)^2,
backward and fused Adam.  Three lines, each 3 warm-up + 10 timed eager steps between device
synchronisations:
  (a) the force step on the HIP path (gmp_amd.energy_and_forces),
  (b) the project's energy-only training step on the same model (forward, L1, backward, Adam),
  (c) the force step with oracle.schnet.SchNetModel moved to the GPU (plain torch ops on the same
      device).
Prints one JSON line and, with --out, writes it to a file.

  python scripts/bench_schnet_forces.py [--nodes N --edges E --steps K --warmup W --out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "geometric-message-passing_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a,b,c", help="comma-joined subset of a, b, c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_schnet_forces: no HIP device (a timing needs the GPU)")

    import gmp_amd
    from gmp_amd.graph import Batch, radius_graph
    from oracle import schnet as osch

    dev = torch.device("cuda:0")
    g = radius_graph(args.nodes, args.edges)
    atoms = torch.ones_like(g.atoms)  # Embedding(100, padding_idx=0): type 1 is a trained row
    gen = torch.Generator().manual_seed(0)
    y = torch.randn(1, 1, generator=gen).to(dev)
    Fs = torch.randn(g.num_nodes, 3, generator=gen).to(dev)
    pos = g.pos.to(dev).requires_grad_(True)
    batch = Batch(atoms.to(dev), pos, g.edge_index.to(dev),
                  torch.zeros(g.num_nodes, dtype=torch.long, device=dev), num_graphs=1)

    def make(mod):
        torch.manual_seed(0)
        model = mod.SchNetModel().to(dev)
        return model, torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)

    def force_step_hip(model, opt):
        def step():
            opt.zero_grad(set_to_none=True)
            E, F = gmp_amd.energy_and_forces(model, batch, create_graph=True)
            ((E - y).abs().sum() + ((F - Fs) ** 2).sum()).backward()
            opt.step()
        return step

    def energy_step(model, opt):
        bd = Batch(batch.atoms, pos.detach(), batch.edge_index, batch.batch, num_graphs=1)

        def step():
            opt.zero_grad(set_to_none=True)
            (model(bd) - y).abs().sum().backward()
            opt.step()
        return step

    def force_step_torch(model, opt):
        def step():
            opt.zero_grad(set_to_none=True)
            E = model(batch)
            (gp,) = torch.autograd.grad(E.sum(), pos, create_graph=True)
            ((E - y).abs().sum() + ((-gp - Fs) ** 2).sum()).backward()
            opt.step()
        return step

    rec = {"workload": "SchNet (defaults) energy-and-force step", "nodes": g.num_nodes,
           "edges": g.num_edges, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    lines = {"a": ("hip_force_step", gmp_amd, force_step_hip),
             "b": ("hip_energy_step", gmp_amd, energy_step),
             "c": ("torch_oracle_force_step", osch, force_step_torch)}
    for key in args.only.split(","):
        name, mod, mk = lines[key]
        model, opt = make(mod)
        ms = timed(mk(model, opt), args.warmup, args.steps)
        rec[name] = {"ms_per_step": round(ms, 3),
                     "edges_per_s": round(g.num_edges / (ms * 1e-3), 1)}
        rec[name]["peak_mem_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        del model, opt
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if "hip_force_step" in rec and "hip_energy_step" in rec:
        rec["force_over_energy"] = round(rec["hip_force_step"]["ms_per_step"]
                                         / rec["hip_energy_step"]["ms_per_step"], 3)
    if "hip_force_step" in rec and "torch_oracle_force_step" in rec:
        rec["oracle_over_hip"] = round(rec["torch_oracle_force_step"]["ms_per_step"]
                                       / rec["hip_force_step"]["ms_per_step"], 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
