"""Microbenchmark of K18 + K19: forward + backward of one SphereNet update_e (hidden 128, int 64,
basis (7, 6), basis_emb 8) on a radius graph of a few million triplets.

fused:    the triplet projections by K18 from jb / angle / torsion (embeddings never in HBM)
          and the triplet interaction by K19;
composed: the reference's formulation on the GPU: materialised angle_emb (T, 42) and
          torsion_emb (T, 294), two Linears each, x_kj[idx_kj] * sbf * t by index_select and
          the sum over idx_ji by index_add_.  The embeddings are built once outside the timed
          window (the reference builds them once per forward and re-reads them in every layer).

The two are timed alternately in one process; the single kernels are timed on their own against
the traffic model below (bytes each must move per triplet).  Prints one JSON line.

    python scripts/mb_spherenet.py [--nodes 20000] [--degree 14] [--iters 10]
    rocprofv3 --kernel-trace --stats -d bench_out/mb_spherenet -- \
        python scripts/mb_spherenet.py --iters 3
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
from gmp_amd.spherenet import swish  # noqa: E402
from gmp_amd.triplets import xyz_to_dat_offsets  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=20000)
ap.add_argument("--degree", type=float, default=14.0)
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()

dev = torch.device("cuda:0")
H, I, n, k, b = 128, 64, 7, 6, 8
r = 2.0
torch.manual_seed(0)
box = (args.nodes * 4.18879 * r ** 3 / args.degree) ** (1 / 3)
pos = torch.rand(args.nodes, 3, device=dev) * box
ei = gmp_amd.radius_graph_gpu(pos, r, max_num_neighbors=None)
dist, angle, torsion, _, _, idx_kj, idx_ji, offs = xyz_to_dat_offsets(pos, ei, args.nodes)
E, T = dist.numel(), angle.numel()

layer = gmp_amd.update_e(H, I, b, b, b, n, k, 1, 2).to(dev)
emb = gmp_amd.emb(n, k, 2.5 * r, 5).to(dev)
with torch.no_grad():
    rbf, jb = emb(dist)
    a_emb, t_emb = ops.sph_triplet_embeddings(jb, angle, torsion, idx_kj, emb.pref, n, k)
x1 = torch.randn(E, H, device=dev)
cot = torch.randn(E, H, device=dev)


def fused():
    S, P = ops.SphTripletProjFn.apply(jb, angle, torsion, idx_kj, emb.pref, n, k, 1,
                                      layer.lin_sbf1.weight, layer.lin_t1.weight)
    return layer(x1, rbf, S, P, idx_kj, idx_ji, offs, want_e2=False)[0]


def composed():
    lin = torch.nn.functional.linear

    def row(m, x):  # the edge-row Linears are the same in both paths
        return ops.linear(x, m.weight, m.bias)

    x_ji = swish(row(layer.lin_ji, x1))
    x_kj = swish(row(layer.lin_kj, x1)) * row(layer.lin_rbf2, row(layer.lin_rbf1, rbf))
    x_kj = swish(row(layer.lin_down, x_kj))
    sbf = lin(lin(a_emb, layer.lin_sbf1.weight), layer.lin_sbf2.weight)
    t = lin(lin(t_emb, layer.lin_t1.weight), layer.lin_t2.weight)
    msg = x_kj.index_select(0, idx_kj) * sbf * t
    m = torch.zeros(E, I, device=dev).index_add_(0, idx_ji, msg)
    e1 = x_ji + swish(row(layer.lin_up, m))
    for res in layer.layers_before_skip:
        e1 = res(e1)
    e1 = swish(row(layer.lin, e1)) + x1
    for res in layer.layers_after_skip:
        e1 = res(e1)
    return e1


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
for _ in range(3):  # alternate: other work shares the machine
    tf.append(timed(lambda: step(fused), args.iters))
    tc.append(timed(lambda: step(composed), args.iters))

# single kernels against the bytes they must move
tops = gmp_amd._lib.torch_ops()
w1t = ops.sph_feature_major([layer.lin_sbf1.weight.detach()], n * k)
w2t = ops.sph_feature_major([layer.lin_t1.weight.detach()], n * n * k)
S, P = tops.sph_triplet_proj_fwd(jb, angle, torsion, idx_kj, emb.pref, w1t, w2t, n, k, 1, b, b)
xd = torch.randn(E, I, device=dev)
gm = torch.randn(E, I, device=dev)
Wa, Wt = layer.lin_sbf2.weight.detach(), layer.lin_t2.weight.detach()
csr = ops.get_csr(idx_kj, E)
kern = {
    # per triplet: the gathered jb row, angle, torsion, idx_kj in; S and P rows out
    "K18 proj fwd": (lambda: tops.sph_triplet_proj_fwd(jb, angle, torsion, idx_kj, emb.pref, w1t,
                                                       w2t, n, k, 1, b, b),
                     T * (4 * n * k + 16 + 8 * b)),
    # the same in, grad S and grad P in, nothing per triplet out
    "K18 proj wgrad": (lambda: tops.sph_triplet_proj_bwd(jb, angle, torsion, idx_kj, emb.pref,
                                                         w1t, w2t, n, k, 1, b, b, S, P, False),
                       T * (4 * n * k + 16 + 8 * b)),
    # per triplet: S, P, idx_kj and the gathered xd row in; per edge one row out
    "K19 fwd": (lambda: tops.triplet_interact_fwd(xd, S[0], P[0], Wa, Wt, idx_kj, None, offs),
                T * (8 * b + 8 + 4 * I) + E * 4 * I),
    # per triplet: S, P, idx_kj, the xd row in, grad S and grad P out; per edge grad_m in
    "K19 bwd (S, P, W)": (lambda: tops.triplet_interact_bwd(gm, xd, S[0], P[0], Wa, Wt, idx_kj,
                                                            offs),
                          T * (16 * b + 8 + 4 * I) + E * 4 * I),
    "K19 bwd (xd)": (lambda: tops.triplet_interact_fwd(gm, S[0], P[0], Wa, Wt, idx_ji, csr.perm,
                                                       csr.rowptr),
                     T * (8 * b + 16 + 4 * I) + E * 4 * I),
}
kernels = {}
for name, (f, nbytes) in kern.items():
    f()
    ms = timed(f, args.iters)
    kernels[name] = {"ms": round(ms, 4), "model_GB": round(nbytes / 1e9, 3),
                     "TB_per_s": round(nbytes / ms / 1e9, 3)}
print(json.dumps({"nodes": args.nodes, "edges": E, "triplets": T,
                  "fused_ms": [round(v, 3) for v in tf], "composed_ms": [round(v, 3) for v in tc],
                  "rel_diff_fused_vs_composed": diff, "kernels": kernels}))
