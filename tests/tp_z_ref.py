"""Plain fp64 torch evaluation of the per-edge z / dz maps of the node-form tensor product (K7,
csrc/gmp_tp.hip: tp_edge_z2_kernel<2|3>, tp_edge_z_gen_kernel and their backwards), and a
restatement of the code paths those kernels choose among.  No project kernel is called here.

Per path p = (l1, l2, lo) with input block offset x_off, multiplicity mul1, CG tensor C_p and
path weight alpha_p, for the sorted edges e in [e0, e1):

    z_p[e - e0, k mul1 + u] = alpha_p sum_ij C_p[i, j, k] X[e, u, i] Y[e, l2 l2 + j]
        X[e, u, i] = x[src_sorted[e], x_off + u (2 l1 + 1) + i],   Y[e, c] = sh[perm[e], c]

and, given dz_p of the same layout,

    dx_edge[e - e0, x_off + u (2 l1 + 1) + i]
        = sum_{p on the block} alpha_p sum_jk C_p[i, j, k] Y[e, l2 l2 + j] dz_p[e - e0, k mul1 + u]
    dY_edge[e - e0, l2 l2 + j]
        = sum_{p with that l2} alpha_p sum_uik C_p[i, j, k] X[e, u, i] dz_p[e - e0, k mul1 + u]

C_p defaults to the fp32 table the kernels read (plan.cg_host) cast to double, so that the table's
own rounding is no part of a kernel's error; alpha_p is the unrounded float64 of the instruction
list.  tests/test_tp_z_host.py pins these sums against oracle.o3.FullyConnectedTensorProduct with
the unrounded float64 CG tensors and checks that plan.cg_host is exactly their fp32 rounding.
"""
import torch

from gmp_amd import o3


def paths(plan):
    """The plan's path table as plain dicts (integers from plan.paths_host, alpha in float64)."""
    out = []
    for P, ins in zip(plan.paths_host, plan.instructions):
        assert (P.l1, P.l2, P.lo, P.mul1) == (ins["l1"], ins["l2"], ins["lo"], ins["mul1"])
        out.append(dict(l1=P.l1, l2=P.l2, lo=P.lo, mul1=P.mul1, x_off=P.x_off, z_off=P.z_off,
                        cg_off=P.cg_off, io=P.io, alpha=float(ins["alpha"])))
    return out


def cg_f64(plan):
    """The unrounded float64 CG tensors, concatenated as plan.cg_host is."""
    return torch.cat([torch.from_numpy(o3.wigner_3j(i["l1"], i["l2"], i["lo"]).reshape(-1).copy())
                      for i in plan.instructions])


def _operands(plan, P, x, sh, src_sorted, perm, e0, e1, cg, absolute):
    d1, d2, d3 = 2 * P["l1"] + 1, 2 * P["l2"] + 1, 2 * P["lo"] + 1
    cg = plan.cg_host.double() if cg is None else cg
    assert cg.dtype == torch.float64 and x.dtype == torch.float64 and sh.dtype == torch.float64
    C = cg[P["cg_off"]:P["cg_off"] + d1 * d2 * d3].view(d1, d2, d3)
    X = x[src_sorted[e0:e1], P["x_off"]:P["x_off"] + P["mul1"] * d1].reshape(-1, P["mul1"], d1)
    Y = sh[perm[e0:e1], P["l2"] ** 2:P["l2"] ** 2 + d2]
    a = P["alpha"]
    if absolute:
        C, X, Y, a = C.abs(), X.abs(), Y.abs(), abs(a)
    return C, X, Y, a


def z_ref(plan, x, sh, src_sorted, perm, e0, e1, cg=None, absolute=False):
    """Per path, the (e1 - e0, (2 lo + 1) * mul1) float64 z rows (k-major, then u)."""
    out = []
    for P in paths(plan):
        C, X, Y, a = _operands(plan, P, x, sh, src_sorted, perm, e0, e1, cg, absolute)
        z = a * torch.einsum("ijk,eui,ej->eku", C, X, Y)
        out.append(z.reshape(e1 - e0, -1))
    return out


def z_abs(plan, x, sh, src_sorted, perm, e0, e1, cg=None):
    """z_ref over absolute values: the magnitude every rounding error is relative to."""
    return z_ref(plan, x, sh, src_sorted, perm, e0, e1, cg, absolute=True)


def dz_ref(plan, x, sh, src_sorted, perm, e0, e1, dz, cg=None):
    """dz: per path, (e1 - e0, (2 lo + 1) * mul1) float64.  Returns dx_edge (ne, in_dim), dY_edge
    (ne, sh_dim) and the same two sums over absolute values.  Entries of dx_edge that no path
    reads are exactly 0."""
    ne = e1 - e0
    res = []
    for absolute in (False, True):
        dx = torch.zeros(ne, plan.in_dim, dtype=torch.float64)
        dY = torch.zeros(ne, plan.sh_dim, dtype=torch.float64)
        for P, g in zip(paths(plan), dz):
            C, X, Y, a = _operands(plan, P, x, sh, src_sorted, perm, e0, e1, cg, absolute)
            d1, d2, d3 = C.shape
            G = g.reshape(ne, d3, P["mul1"])
            G = G.abs() if absolute else G
            dx[:, P["x_off"]:P["x_off"] + P["mul1"] * d1] += \
                a * torch.einsum("ijk,ej,eku->eui", C, Y, G).reshape(ne, -1)
            dY[:, P["l2"] ** 2:P["l2"] ** 2 + d2] += a * torch.einsum("ijk,eui,eku->ej", C, X, G)
        res += [dx, dY]
    return res[0], res[1], res[2], res[3]


def add_counts(plan):
    """The fp32 additions that feed one output entry, from the path table: per path for z
    ((2 l1 + 1) + (2 l2 + 1)), per input entry for dx (the sum of (2 l2 + 1) + (2 lo + 1) over the
    paths reading its block; 0 where no path does) and per SH component for dY (the sum of
    mul1 (2 l1 + 1) (2 lo + 1) over the paths with that l2)."""
    nz = []
    ndx = torch.zeros(plan.in_dim, dtype=torch.float64)
    ndY = torch.zeros(plan.sh_dim, dtype=torch.float64)
    for P in paths(plan):
        d1, d2, d3 = 2 * P["l1"] + 1, 2 * P["l2"] + 1, 2 * P["lo"] + 1
        nz.append(d1 + d2)
        ndx[P["x_off"]:P["x_off"] + P["mul1"] * d1] += d2 + d3
        ndY[P["l2"] ** 2:P["l2"] ** 2 + d2] += P["mul1"] * d1 * d3
    return nz, ndx, ndY


def z_route(plan):
    """Which code path the z / dz kernels take for this plan.  Restates, from plan.l_max,
    plan.sh_dim and plan.paths_host, these decisions of csrc/gmp_tp.hip:

      kernel     the two launchers gmp_tp_edge_z_lmax_f32 / gmp_tp_edge_z_bwd_lmax_f32
                 ("if (l_max > 3 || d.sh_dim > kMaxSh) .. else if (l_max <= 2 && d.sh_dim <= 9)")
      pre        tp_edge_z2_kernel: "bool pre = LM == 2" and the loop over the path table below it
                 (one input block per l1 <= 2: the sender row is preloaded)
      grouped    tp_edge_z2_bwd_kernel: "grouped |= xoff[P.l1] >= 0 && xoff[P.l1] != P.x_off"
                 (a repeated l in the input irreps; the generic dz kernel has no such branch, the
                 flag then only says that the plan has a repeated l)
      uncovered  tp_edge_z2_bwd_kernel "if (covered != d.in_dim)" and the "if (!in)" loop of
                 tp_edge_z_gen_bwd_kernel: input entries that no path reads
      mul_halves z_path / z_path_pre / z_bwd_path "u = lane + 64 * uu; if (u < P.mul1)" and the
                 generic kernels' "for (u = lane; u < P.mul1; u += 64)": per distinct mul1,
                 "one" (<= 64), "partial" (65..127) or "full" (128)
    """
    P = paths(plan)
    if plan.l_max > 3 or plan.sh_dim > 16:
        kernel = "gen"
    elif plan.l_max <= 2 and plan.sh_dim <= 9:
        kernel = "z2<2>"
    else:
        kernel = "z2<3>"
    xo, pre = {}, kernel == "z2<2>"
    for p in P:
        if p["l1"] > 2 or (p["l1"] in xo and xo[p["l1"]] != p["x_off"]):
            pre = False
        else:
            xo[p["l1"]] = p["x_off"]
    xoff, grouped = {}, False
    for p in P:
        grouped |= p["l1"] in xoff and xoff[p["l1"]] != p["x_off"]
        xoff[p["l1"]] = p["x_off"]
    blocks = {p["x_off"]: p["mul1"] * (2 * p["l1"] + 1) for p in P}
    muls = {p["x_off"]: p["mul1"] for p in P}
    halves = {m: "one" if m <= 64 else "partial" if m < 128 else "full" for m in muls.values()}
    return dict(kernel=kernel, pre=pre, grouped=bool(grouped),
                uncovered=plan.in_dim - sum(blocks.values()), mul_halves=halves,
                ragged=len(set(muls.values())) > 1, l1_max=max(p["l1"] for p in P),
                n_paths=len(P))
