"""Microbenchmark of K18d + K19d: forward + backward of one DimeNet++ InteractionPPBlock (hidden
128, int 64, basis (7, 6), basis_emb 8) on a radius graph of a few million triplets.

fused:    the triplet projection by K18d from sbe / angle (the embedding never in HBM) and the
          triplet interaction by K19d;
composed: PyG's formulation on this project's own ops: the materialised sbf (T, 42) from
          gmp_dime_triplet_emb, built once outside the timed window (PyG builds it once per
          forward and re-reads it in every block), two ops.linear, x_kj[idx_kj] * sbf by
          index_select and the sum over idx_ji by index_add_.

The two are timed alternately in one process (device events, three warm-up steps); the single
kernels are timed on their own against the traffic model below (bytes each must move per
triplet), K19's gradient kernel on the same graph beside K19d's.  Prints one JSON line.

    python scripts/mb_dimenet.py [--nodes 20000] [--degree 14] [--iters 10] [--windows 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "geometric-message-passing_amd"))
import gmp_amd  # noqa: E402
from gmp_amd import ops  # noqa: E402
from gmp_amd.dimenet import InteractionPPBlock  # noqa: E402
from gmp_amd.spherenet import swish  # noqa: E402
from gmp_amd.triplets import dimenet_angles, triplet_offsets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=20000)
ap.add_argument("--degree", type=float, default=14.0)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--windows", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
H, I, n, k, b = 128, 64, 7, 6, 8
r = 2.0
torch.manual_seed(0)
box = (args.nodes * 4.18879 * r ** 3 / args.degree) ** (1 / 3)
pos = torch.rand(args.nodes, 3, device=dev) * box
ei = gmp_amd.radius_graph_gpu(pos, r, max_num_neighbors=None)
dist, angle, _, _, _, _, _, idx_kj, idx_ji = dimenet_angles(pos, ei, args.nodes)
E, T = dist.numel(), angle.numel()
offs = triplet_offsets(idx_ji, E)

model = gmp_amd.DimeNetPPModel(hidden_channels=H, int_emb_size=I, basis_emb_size=b,
                               num_spherical=n, num_radial=k, cutoff=2.5 * r, num_layers=1).to(dev)
layer = model.interaction_blocks[0]
assert isinstance(layer, InteractionPPBlock)
pref = model.sbf.pref
with torch.no_grad():
    rbf, sbe = model.bases(dist)
    sbf = ops.dime_triplet_embeddings(sbe, angle, idx_kj, pref, n, k)
x1 = torch.randn(E, H, device=dev)
cot = torch.randn(E, H, device=dev)


def fused():
    (S,) = ops.DimeTripletProjFn.apply(sbe, angle, idx_kj, pref, n, k, 1, layer.lin_sbf1.weight)
    return layer(x1, rbf, S, idx_kj, idx_ji, offs)


def composed():
    def row(m, x):  # the edge-row Linears are the same in both paths
        return ops.linear(x, m.weight, m.bias)

    x_ji = swish(row(layer.lin_ji, x1))
    x_kj = swish(row(layer.lin_kj, x1)) * row(layer.lin_rbf2, row(layer.lin_rbf1, rbf))
    x_kj = swish(row(layer.lin_down, x_kj))
    s = ops.linear(ops.linear(sbf, layer.lin_sbf1.weight), layer.lin_sbf2.weight)
    msg = x_kj.index_select(0, idx_kj) * s
    m = torch.zeros(E, I, device=dev).index_add_(0, idx_ji, msg)
    h = x_ji + swish(row(layer.lin_up, m))
    for res in layer.layers_before_skip:
        h = res(h)
    h = swish(row(layer.lin, h)) + x1
    for res in layer.layers_after_skip:
        h = res(h)
    return h


def step(f):
    layer.zero_grad(set_to_none=True)
    out = f()
    (out * cot).sum().backward()
    return out


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for _ in range(3):
    of, oc = step(fused), step(composed)
diff = float((of - oc).detach().abs().max() / oc.detach().abs().max())
tf, tc = [], []
for _ in range(max(3, args.windows)):  # alternate: other work shares the machine
    tf.append(timed(lambda: step(fused), args.iters))
    tc.append(timed(lambda: step(composed), args.iters))

# single kernels against the bytes they must move
tops = gmp_amd._lib.torch_ops()
wt = ops.sph_feature_major([layer.lin_sbf1.weight.detach()], n * k)
S = tops.dime_triplet_proj_fwd(sbe, angle, idx_kj, pref, wt, n, k, 1, b)
xd = torch.randn(E, I, device=dev)
gm = torch.randn(E, I, device=dev)
W = layer.lin_sbf2.weight.detach()
gS = torch.randn(1, T, b, device=dev)
g_rbf, g_sbe = torch.randn_like(rbf), torch.randn_like(sbe)
freq, zeros, norm = model.rbf.freq.detach(), model.sbf.zeros, model.sbf.norm
cutoff, p = float(model.cutoff), int(model.envelope_exponent)
csr = ops.get_csr(idx_kj, E)
nk = n * k
kern = {
    # per edge: dist in, the rbf and sbe rows out
    "K18d edge fwd": (lambda: tops.dime_edge_basis_fwd(dist, freq, zeros, norm, cutoff, p),
                      E * (4 + 4 * k + 4 * nk)),
    # per edge: dist and both gradient rows in, grad_dist out
    "K18d edge bwd": (lambda: tops.dime_edge_basis_bwd(dist, freq, zeros, norm, cutoff, p, g_rbf,
                                                       g_sbe),
                      E * (8 + 4 * k + 4 * nk)),
    # per triplet: the gathered sbe row, angle, idx_kj in; the S row out
    "K18d proj fwd": (lambda: tops.dime_triplet_proj_fwd(sbe, angle, idx_kj, pref, wt, n, k, 1, b),
                      T * (4 * nk + 12 + 4 * b)),
    # the same in, grad S in, nothing per triplet out
    "K18d proj wgrad": (lambda: tops.dime_triplet_proj_bwd(sbe, angle, idx_kj, pref, wt, n, k, 1,
                                                           b, gS, False),
                        T * (4 * nk + 12 + 4 * b)),
    # wgrad plus the geometry pass: the same in again, grad_sbe_rows and grad_angle out
    "K18d proj bwd (w, sbe, angle)": (lambda: tops.dime_triplet_proj_bwd(sbe, angle, idx_kj, pref,
                                                                         wt, n, k, 1, b, gS, True),
                                      T * (2 * (4 * nk + 12 + 4 * b) + 4 * nk + 4)),
    # the materialised sbf (the composed path's input): the same in, the sbf row out
    "K18d emb": (lambda: tops.dime_triplet_emb(sbe, angle, idx_kj, pref, n, k),
                 T * (4 * nk + 12 + 4 * nk)),
    # per triplet: S, idx_kj and the gathered xd row in; per edge one row out
    "K19d fwd": (lambda: tops.triplet_interact1_fwd(xd, S[0], W, idx_kj, None, offs),
                 T * (4 * b + 8 + 4 * I) + E * 4 * I),
    # per triplet: S, idx_kj, the xd row in, grad S out; per edge grad_m in
    "K19d bwd (S, W)": (lambda: tops.triplet_interact1_bwd(gm, xd, S[0], W, idx_kj, offs),
                        T * (8 * b + 8 + 4 * I) + E * 4 * I),
    "K19d bwd (xd)": (lambda: tops.triplet_interact1_fwd(gm, S[0], W, idx_ji, csr.perm,
                                                         csr.rowptr),
                      T * (4 * b + 16 + 4 * I) + E * 4 * I),
    # K19's gradient kernel (two factors) on the same graph, P a second copy of S's shape
    "K19 bwd (S, P, W)": (lambda: tops.triplet_interact_bwd(gm, xd, S[0], gS[0], W, W, idx_kj,
                                                            offs),
                          T * (16 * b + 8 + 4 * I) + E * 4 * I),
}
kernels = {}
for name, (f, nbytes) in kern.items():
    f()
    ms = sorted(timed(f, args.iters) for _ in range(3))
    kernels[name] = {"ms": [round(v, 4) for v in ms], "model_GB": round(nbytes / 1e9, 3),
                     "TB_per_s": round(nbytes / ms[0] / 1e9, 3)}
print(json.dumps({"nodes": args.nodes, "edges": E, "triplets": T,
                  "fused_ms": [round(v, 3) for v in tf], "composed_ms": [round(v, 3) for v in tc],
                  "rel_diff_fused_vs_composed": diff, "kernels": kernels}))
