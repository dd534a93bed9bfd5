"""Triplet enumeration and angle / torsion featurisation on the device (K11; SURVEY.md §8(f) f3,
the "angles" of the north star's featurisation list).

`xyz_to_dat` mirrors models/layers/spherenet_layer.py:496-564 (same arguments, same returns);
`dimenet_triplets` / `dimenet_angles` mirror the DimeNet forward models/dimenet.py:79-90 (PyG
DimeNet.triplets).  The reference builds the triplets with torch_sparse (a SparseTensor by
target, row-selected by source); here the adjacency by (target, source) comes from two stable
CSR builds (K0), and K11 counts, then fills the triplets with their angles (and SphereNet
torsions) in one pass, in the reference's order.

Distances and angles are differentiable w.r.t. `pos` (PyG DimeNet differentiates its angles,
dimenet.py:79-90, e.g. for forces): the backward kernel gmp_triplet_geom_bwd_f32 writes one
gradient row per (triplet, corner) and per (edge, end), summed per node over a CSR
(deterministic).  The SphereNet torsion (a scatter-min over candidates k_n,
spherenet_layer.py:535-559) is differentiable too: the fill kernel records the winning k_n of
every triplet and gmp_triplet_torsion_bwd_f32 routes the gradient to that candidate only, as
torch_scatter's scatter_min backward does (first index among equal minima).

Periodic graphs (K11p, the contract of include/gmp.h) run in edge-vector form: the image-aware
lists from shift_idx, dist / angle (and, for SphereNet, the torsion over the triplets of the same
edge) from vec = (pos[j] - pos[i]) + shift, and backward kernels that return per-edge gradients
summed over cached CSRs; pos and the cell are reached through the recorded linear maps.
"""
import torch

from . import _lib, ops
from .graph import edge_shift


def adjacency_by_target(edge_index, num_nodes):
    """Entries of edge_index sorted by (target, source), stable in edge id:
    rowptr (N+1), source per entry, edge id per entry."""
    src, dst = ops._i64c(edge_index[0]), ops._i64c(edge_index[1])
    by_src = ops.CSR(src, num_nodes)
    by_dst = ops.CSR(dst[by_src.perm], num_nodes)
    order = by_src.perm[by_dst.perm]
    return by_dst.rowptr, src[order], order


def _cot(g):
    """A cotangent for a kernel: contiguous float32, or None kept as None (a NULL pointer)."""
    return ops._f32c(g) if g is not None else None


def _enumerate(ei, num_nodes, count, fill):
    """The enumeration shared by K11 and K11p: adjacency by target, count(adj, counts, stream),
    the triplet offsets, the one host read of T, the lists, fill(adj, offs, T, idx_kj, idx_ji,
    stream).  -> idx_kj, idx_ji, offs, and what fill returns (the per-triplet arrays it made)."""
    E, dev = ei.shape[1], ei.device
    adj = adjacency_by_target(ei, num_nodes)
    counts = torch.empty(E, dtype=torch.int64, device=dev)
    s = ops._stream()
    count(adj, counts, s)
    offs = torch.zeros(E + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offs[1:])
    T = int(offs[-1].item()) if E else 0
    idx_kj = torch.empty(T, dtype=torch.int64, device=dev)
    idx_ji = torch.empty(T, dtype=torch.int64, device=dev)
    return idx_kj, idx_ji, offs, fill(adj, offs, T, idx_kj, idx_ji, s)


def _run(pos, edge_index, num_nodes, mode, want_angle, want_torsion, want_dist, want_kn=False):
    lib = _lib.load()
    ei = ops._i64c(edge_index)
    ops._need_cuda(ei)
    if pos is not None:
        pos = ops._f32c(pos.detach())
        ops._need_cuda(pos)
    dev = ei.device
    E = ei.shape[1]
    N = int(num_nodes)
    dist = torch.empty(E, dtype=torch.float32, device=dev) if want_dist else None

    def count(adj, counts, s):
        ops.check(lib.gmp_triplet_count(ops._p(pos), ops._p(ei), E, N, ops._p(adj[0]),
                                        ops._p(adj[1]), ops._p(counts), ops._p(dist), s),
                  "gmp_triplet_count")

    def fill(adj, offs, T, idx_kj, idx_ji, s):
        angle = torch.empty(T, dtype=torch.float32, device=dev) if want_angle else None
        torsion = torch.empty(T, dtype=torch.float32, device=dev) if want_torsion else None
        kn = torch.empty(T, dtype=torch.int64, device=dev) if want_kn else None
        ops.check(lib.gmp_triplet_fill_f32(ops._p(pos), ops._p(ei), E, N, *map(ops._p, adj),
                                           ops._p(offs), T, mode, ops._p(idx_kj), ops._p(idx_ji),
                                           ops._p(angle), ops._p(torsion), ops._p(kn), s),
                  "gmp_triplet_fill_f32")
        return angle, torsion, kn

    idx_kj, idx_ji, _, (angle, torsion, kn) = _enumerate(ei, N, count, fill)
    if want_kn:
        return dist, angle, torsion, idx_kj, idx_ji, kn
    return dist, angle, torsion, idx_kj, idx_ji


def _geom_forward(ctx, pos, edge_index, num_nodes, mode, use_torsion):
    """The forward of TripletGeomFn and TripletGeom2Fn: torsion and its winners k_n are empty
    without use_torsion."""
    res = _run(pos, edge_index, num_nodes, mode, True, use_torsion, True, use_torsion)
    dist, angle, torsion, idx_kj, idx_ji = res[:5]
    kn = res[5] if use_torsion else None
    if torsion is None:
        torsion = torch.empty(0, dtype=torch.float32, device=dist.device)
        kn = torch.empty(0, dtype=torch.int64, device=dist.device)
    ctx.save_for_backward(pos, ops._i64c(edge_index), idx_kj, idx_ji, kn)
    ctx.mode, ctx.n, ctx.use_torsion = mode, int(num_nodes), use_torsion
    ctx.mark_non_differentiable(idx_kj, idx_ji)
    return dist, angle, torsion, idx_kj, idx_ji


def _geom_bwd_rows(pos, ei, idx_kj, idx_ji, g_dist, g_angle, mode, spare=0):
    """rows (3T + 2E + spare, 3) and node of gmp_triplet_geom_bwd_f32; the spare rows at the end
    are left for the torsion's."""
    E, T = ei.shape[1], idx_kj.numel()
    rows, node = _geom_rows(3 * T + 2 * E + spare, pos.device)
    gd, ga, p32 = _cot(g_dist), _cot(g_angle), ops._f32c(pos)
    ops.check(_lib.load().gmp_triplet_geom_bwd_f32(
        ops._p(p32), ops._p(ei), E, ops._p(idx_kj), ops._p(idx_ji), T, mode, ops._p(gd),
        ops._p(ga), ops._p(rows), ops._p(node), ops._stream()), "gmp_triplet_geom_bwd_f32")
    return rows, node


class TripletGeomFn(torch.autograd.Function):
    """(dist (E), angle (T), torsion (T, or empty without use_torsion), idx_kj, idx_ji) with the
    backward of dist, angle and torsion w.r.t. pos."""
    forward = staticmethod(_geom_forward)

    @staticmethod
    def backward(ctx, g_dist, g_angle, g_torsion, _g1, _g2):
        pos, ei, idx_kj, idx_ji, kn = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        E, T = ei.shape[1], idx_kj.numel()
        p32 = ops._f32c(pos.detach())
        nt = 4 * T if (ctx.use_torsion and g_torsion is not None) else 0
        rows, node = _geom_bwd_rows(p32, ei, idx_kj, idx_ji, g_dist, g_angle, ctx.mode, nt)
        if nt:
            m = 3 * T + 2 * E
            ops.check(_lib.load().gmp_triplet_torsion_bwd_f32(
                ops._p(p32), ops._p(ei), E, ops._p(idx_kj), ops._p(idx_ji), ops._p(kn), T,
                ops._p(_cot(g_torsion)), ops._p(rows[m:]), ops._p(node[m:]), ops._stream()),
                "gmp_triplet_torsion_bwd_f32")
        return _rows_to_pos(rows, node, ctx.n, pos.dtype), None, None, None, None


class TripletGeom2Fn(torch.autograd.Function):
    """TripletGeomFn (without torsion) whose backward is recorded (TripletGeomBwdFn), so that
    d pos can be differentiated once more: energy-and-force training."""

    @staticmethod
    def forward(ctx, pos, edge_index, num_nodes, mode):
        ctx.set_materialize_grads(False)
        return _geom_forward(ctx, pos, edge_index, num_nodes, mode, False)

    @staticmethod
    def backward(ctx, g_dist, g_angle, _g0, _g1, _g2):
        pos, ei, idx_kj, idx_ji, _ = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_dist is None and g_angle is None):
            return None, None, None, None
        g_pos = TripletGeomBwdFn.apply(pos, ei, idx_kj, idx_ji, g_dist, g_angle, ctx.mode, ctx.n)
        return g_pos, None, None, None


def _geom_rows(n_rows, dev):
    return (torch.empty((n_rows, 3), dtype=torch.float32, device=dev),
            torch.empty(n_rows, dtype=torch.int64, device=dev))


def _rows_to_pos(rows, node, n, dtype):
    """The deterministic segmented sum of the gradient rows by node (zeros without rows)."""
    if rows.shape[0] == 0:
        return torch.zeros((n, 3), dtype=dtype, device=rows.device)
    return ops.segment_reduce(rows, ops.CSR(node, n), "sum")[0].to(dtype)


class TripletGeomBwdFn(torch.autograd.Function):
    """d pos (N, 3) from pos and the cotangents g_dist (E) / g_angle (T), each possibly None
    (gmp_triplet_geom_bwd_f32 and the segmented sum by node); backward by
    gmp_triplet_geom_bwd2_f32.  The tensors given are saved as they are (a copy made here would
    be cut off from the graph).  The second backward is once-differentiable."""

    @staticmethod
    def forward(ctx, pos, ei, idx_kj, idx_ji, g_dist, g_angle, mode, n):
        ctx.save_for_backward(pos, ei, idx_kj, idx_ji, g_dist, g_angle)
        ctx.mode, ctx.n = mode, n
        rows, node = _geom_bwd_rows(pos, ei, idx_kj, idx_ji, g_dist, g_angle, mode)
        return _rows_to_pos(rows, node, n, pos.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, a_pos):
        pos, ei, idx_kj, idx_ji, g_dist, g_angle = ctx.saved_tensors
        E, T = ei.shape[1], idx_kj.numel()
        dev = pos.device
        need = ctx.needs_input_grad
        rows, node = _geom_rows(3 * T + 2 * E, dev)
        gg_d = torch.empty(E, dtype=torch.float32, device=dev)
        gg_a = torch.empty(T, dtype=torch.float32, device=dev)
        gd, ga = _cot(g_dist), _cot(g_angle)
        p32, a32 = ops._f32c(pos), ops._f32c(a_pos)
        ops.check(_lib.load().gmp_triplet_geom_bwd2_f32(
            ops._p(p32), ops._p(ei), E, ops._p(idx_kj), ops._p(idx_ji), T, ctx.mode, ops._p(gd),
            ops._p(ga), ops._p(a32), ops._p(gg_d), ops._p(gg_a), ops._p(rows), ops._p(node),
            ops._stream()), "gmp_triplet_geom_bwd2_f32")
        h_pos = _rows_to_pos(rows, node, ctx.n, pos.dtype) if need[0] else None
        return (h_pos, None, None, None, gg_d if g_dist is not None and need[4] else None,
                gg_a if g_angle is not None and need[5] else None, None, None)


# --------------------------------------------------------------------------- periodic (K11p)
def _run_pbc(vec, edge_index, num_nodes, shift_idx, want_angle=True, want_dist=True,
             want_offsets=False):
    """K11p (include/gmp.h): the image-aware triplets of a periodic graph with dist / angle from
    the per-edge vectors vec (E, 3); vec None: the lists only.  -> dist, angle, idx_kj, idx_ji
    (and, with want_offsets, the triplet offsets (E + 1))."""
    lib = _lib.load()
    ei = ops._i64c(edge_index)
    ops._need_cuda(ei, shift_idx)
    E = ei.shape[1]
    if tuple(shift_idx.shape) != (E, 3):
        raise ValueError(f"shift_idx of shape {tuple(shift_idx.shape)}, expected ({E}, 3)")
    sidx = shift_idx.to(torch.int32).contiguous()
    if vec is not None:
        vec = ops._f32c(vec.detach())
        ops._need_cuda(vec)
        if tuple(vec.shape) != (E, 3):
            raise ValueError(f"vec of shape {tuple(vec.shape)}, expected ({E}, 3)")
    else:
        want_angle = want_dist = False
    dev = ei.device
    N = int(num_nodes)
    if E == 0:  # nothing to launch
        i64 = torch.empty(0, dtype=torch.int64, device=dev)
        f32 = torch.empty(0, dtype=torch.float32, device=dev)
        out = (f32 if want_dist else None, f32.clone() if want_angle else None, i64, i64.clone())
        return out + (torch.zeros(1, dtype=torch.int64, device=dev),) if want_offsets else out
    dist = torch.empty(E, dtype=torch.float32, device=dev) if want_dist else None

    def count(adj, counts, s):
        ops.check(lib.gmp_triplet_count_pbc(ops._p(vec), ops._p(ei), E, N, *map(ops._p, adj),
                                            ops._p(sidx), ops._p(counts), ops._p(dist), s),
                  "gmp_triplet_count_pbc")

    def fill(adj, offs, T, idx_kj, idx_ji, s):
        angle = torch.empty(T, dtype=torch.float32, device=dev) if want_angle else None
        ops.check(lib.gmp_triplet_fill_pbc_f32(ops._p(vec), ops._p(ei), E, N, *map(ops._p, adj),
                                               ops._p(sidx), ops._p(offs), T, ops._p(idx_kj),
                                               ops._p(idx_ji), ops._p(angle), s),
                  "gmp_triplet_fill_pbc_f32")
        return angle

    idx_kj, idx_ji, offs, angle = _enumerate(ei, N, count, fill)
    if want_offsets:
        return dist, angle, idx_kj, idx_ji, offs
    return dist, angle, idx_kj, idx_ji


def _rows_to_vec(rows, idx_kj, idx_ji, E, dtype):
    """g_vec (E, 3) from the (2T + E, 3) rows of the vector-form kernels: the per-edge rows, plus
    the rows of edge idx_ji[t] summed over the triplet offsets, plus the rows of edge idx_kj[t]
    summed over the CSR of idx_kj (both cached per graph; deterministic)."""
    T = idx_kj.numel()
    g = rows[2 * T:]
    if T:
        own, _ = ops.segment_reduce(rows[:T], ops.get_csr(idx_ji, E), "sum", use_perm=False)
        g = g + own + ops._sum_rows_per_edge(rows[T:2 * T], idx_kj, g)
    return g.to(dtype)


def _vec_bwd(vec, idx_kj, idx_ji, g_dist, g_angle):
    E, T = vec.shape[0], idx_kj.numel()
    rows = torch.empty((2 * T + E, 3), dtype=torch.float32, device=vec.device)
    gd, ga = _cot(g_dist), _cot(g_angle)
    ops.check(_lib.load().gmp_triplet_vec_bwd_f32(
        ops._p(ops._f32c(vec)), E, ops._p(idx_kj), ops._p(idx_ji), T, ops._p(gd), ops._p(ga),
        ops._p(rows), ops._stream()), "gmp_triplet_vec_bwd_f32")
    return _rows_to_vec(rows, idx_kj, idx_ji, E, vec.dtype)


def _vec_geom_forward(ctx, vec, edge_index, num_nodes, shift_idx):
    """The forward of TripletVecGeomFn and TripletVecGeom2Fn."""
    dist, angle, idx_kj, idx_ji = _run_pbc(vec, edge_index, num_nodes, shift_idx)
    ctx.save_for_backward(vec, idx_kj, idx_ji)
    ctx.mark_non_differentiable(idx_kj, idx_ji)
    ctx.set_materialize_grads(False)
    return dist, angle, idx_kj, idx_ji


class TripletVecGeomFn(torch.autograd.Function):
    """(dist (E), angle (T), idx_kj, idx_ji) of K11p from vec (E, 3) with the backward of dist and
    angle w.r.t. vec (gmp_triplet_vec_bwd_f32); once differentiable."""
    forward = staticmethod(_vec_geom_forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dist, g_angle, _g1, _g2):
        vec, idx_kj, idx_ji = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_dist is None and g_angle is None):
            return None, None, None, None
        return _vec_bwd(vec, idx_kj, idx_ji, g_dist, g_angle), None, None, None


class TripletVecGeom2Fn(torch.autograd.Function):
    """TripletVecGeomFn whose backward is recorded (TripletVecGeomBwdFn), so that d vec can be
    differentiated once more: energy-and-force training on a periodic structure."""
    forward = staticmethod(_vec_geom_forward)

    @staticmethod
    def backward(ctx, g_dist, g_angle, _g1, _g2):
        vec, idx_kj, idx_ji = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (g_dist is None and g_angle is None):
            return None, None, None, None
        return TripletVecGeomBwdFn.apply(vec, idx_kj, idx_ji, g_dist, g_angle), None, None, None


class TripletVecGeomBwdFn(torch.autograd.Function):
    """d vec (E, 3) from vec and the cotangents g_dist (E) / g_angle (T), each possibly None
    (gmp_triplet_vec_bwd_f32 and the per-edge sums); backward by gmp_triplet_vec_bwd2_f32.  The
    tensors given are saved as they are (a copy made here would be cut off from the graph).  The
    second backward is once-differentiable."""

    @staticmethod
    def forward(ctx, vec, idx_kj, idx_ji, g_dist, g_angle):
        ctx.save_for_backward(vec, idx_kj, idx_ji, g_dist, g_angle)
        return _vec_bwd(vec, idx_kj, idx_ji, g_dist, g_angle)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, a_vec):
        vec, idx_kj, idx_ji, g_dist, g_angle = ctx.saved_tensors
        E, T = vec.shape[0], idx_kj.numel()
        dev = vec.device
        need = ctx.needs_input_grad
        rows = torch.empty((2 * T + E, 3), dtype=torch.float32, device=dev)
        gg_d = torch.empty(E, dtype=torch.float32, device=dev)
        gg_a = torch.empty(T, dtype=torch.float32, device=dev)
        gd, ga = _cot(g_dist), _cot(g_angle)
        ops.check(_lib.load().gmp_triplet_vec_bwd2_f32(
            ops._p(ops._f32c(vec)), E, ops._p(idx_kj), ops._p(idx_ji), T, ops._p(gd), ops._p(ga),
            ops._p(ops._f32c(a_vec)), ops._p(gg_d), ops._p(gg_a), ops._p(rows), ops._stream()),
            "gmp_triplet_vec_bwd2_f32")
        h_vec = _rows_to_vec(rows, idx_kj, idx_ji, E, vec.dtype) if need[0] else None
        return (h_vec, None, None, gg_d if g_dist is not None and need[3] else None,
                gg_a if g_angle is not None and need[4] else None)


def _run_dat_pbc(vec, edge_index, num_nodes, shift_idx, use_torsion):
    """SphereNet's geometry on a periodic graph (K11p, include/gmp.h): K11p's count and fill for
    the lists and dist (angle = NULL), then gmp_triplet_dat_pbc_f32 for the angle at j and the
    torsion with its winner.  -> dist, angle, torsion, idx_kj, idx_ji, offsets, torsion_arg
    (torsion / torsion_arg None without use_torsion)."""
    dist, _, idx_kj, idx_ji, offs = _run_pbc(vec, edge_index, num_nodes, shift_idx,
                                             want_angle=False, want_offsets=True)
    E, T = dist.numel(), idx_kj.numel()
    dev = dist.device
    angle = torch.empty(T, dtype=torch.float32, device=dev)
    torsion = torch.empty(T, dtype=torch.float32, device=dev) if use_torsion else None
    arg = torch.empty(T, dtype=torch.int64, device=dev) if use_torsion else None
    v32 = ops._f32c(vec.detach())
    ops.check(_lib.load().gmp_triplet_dat_pbc_f32(
        ops._p(v32), E, ops._p(idx_kj), ops._p(idx_ji), ops._p(offs), T, ops._p(angle),
        ops._p(torsion), ops._p(arg), ops._stream()), "gmp_triplet_dat_pbc_f32")
    return dist, angle, torsion, idx_kj, idx_ji, offs, arg


class TripletVecDatFn(torch.autograd.Function):
    """(dist (E), angle (T, vertex j), torsion (T, or empty without use_torsion), idx_kj, idx_ji)
    of SphereNet on a periodic graph from vec (E, 3), with the backward of dist, angle and torsion
    w.r.t. vec (gmp_triplet_dat_vec_bwd_f32, the scatter-min's winner held fixed); once
    differentiable."""

    @staticmethod
    def forward(ctx, vec, edge_index, num_nodes, shift_idx, use_torsion):
        dist, angle, torsion, idx_kj, idx_ji, offs, arg = _run_dat_pbc(
            vec, edge_index, num_nodes, shift_idx, use_torsion)
        if torsion is None:
            torsion = torch.empty(0, dtype=torch.float32, device=dist.device)
            arg = torch.empty(0, dtype=torch.int64, device=dist.device)
        ctx.save_for_backward(vec, idx_kj, idx_ji, offs, arg)
        ctx.use_torsion = use_torsion
        ctx.mark_non_differentiable(idx_kj, idx_ji)
        ctx.set_materialize_grads(False)
        return dist, angle, torsion, idx_kj, idx_ji

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dist, g_angle, g_torsion, _g1, _g2):
        vec, idx_kj, idx_ji, offs, arg = ctx.saved_tensors
        if not ctx.use_torsion:
            g_torsion = None
        if not ctx.needs_input_grad[0] or (g_dist is None and g_angle is None
                                           and g_torsion is None):
            return None, None, None, None, None
        E, T = vec.shape[0], idx_kj.numel()
        rows = torch.empty((2 * T + E, 3), dtype=torch.float32, device=vec.device)
        gd, ga, gt = _cot(g_dist), _cot(g_angle), _cot(g_torsion)
        ops.check(_lib.load().gmp_triplet_dat_vec_bwd_f32(
            ops._p(ops._f32c(vec)), E, ops._p(idx_kj), ops._p(idx_ji), ops._p(offs), ops._p(arg),
            T, ops._p(gd), ops._p(ga), ops._p(gt), ops._p(rows), ops._stream()),
            "gmp_triplet_dat_vec_bwd_f32")
        return _rows_to_vec(rows, idx_kj, idx_ji, E, vec.dtype), None, None, None, None


def _dat_pbc(vec, edge_index, num_nodes, shift_idx, use_torsion):
    if vec.requires_grad and torch.is_grad_enabled():
        return TripletVecDatFn.apply(vec, edge_index, num_nodes, shift_idx, use_torsion)
    return _run_dat_pbc(vec, edge_index, num_nodes, shift_idx, use_torsion)[:5]


def edge_vectors(pos, edge_index, shift):
    """vec (E, 3) = (pos[j] - pos[i]) + t, the K9p contract's featurised vector, in recorded ops
    (EdgePosDiffFn and an add: differentiable in pos and shift to any order)."""
    return ops.EdgePosDiffFn.apply(pos, ops._i64c(edge_index)) + shift


def model_geometry_inputs(name, model, batch, first_order_only):
    """The opening of a triplet model's forward: -> pos, shift, shift_idx for xyz_to_dat /
    dimenet_angles.  A batch with edge_shift_idx needs model.periodic (NotImplementedError in the
    model's `name`) and batch.cell (edge_shift's ValueError), both before any device work; with
    first_order_only, pos and shift pass through FirstOrderOnlyFn (forces / stress yes, training
    through them no)."""
    shift_idx = getattr(batch, "edge_shift_idx", None)
    shift = None
    if shift_idx is not None:
        if not getattr(model, "periodic", False):
            raise NotImplementedError(
                f"{name}: periodic shifts (edge_shift_idx) need a model built (or set) with "
                "periodic=True: K11's open-boundary triplets take no periodic images")
        shift = edge_shift(batch)
    pos = batch.pos
    ops._need_cuda(batch.atoms, pos, batch.edge_index, batch.batch)
    if first_order_only and torch.is_grad_enabled():
        if pos.requires_grad:
            pos = ops.FirstOrderOnlyFn.apply(pos)
        if shift is not None and shift.requires_grad:
            shift = ops.FirstOrderOnlyFn.apply(shift)
    return pos, shift, shift_idx


def _geom_pbc(vec, edge_index, num_nodes, shift_idx, twice=False):
    if vec.requires_grad and torch.is_grad_enabled():
        fn = TripletVecGeom2Fn if twice else TripletVecGeomFn
        return fn.apply(vec, edge_index, num_nodes, shift_idx)
    return _run_pbc(vec, edge_index, num_nodes, shift_idx)


def _geom(pos, edge_index, num_nodes, mode, use_torsion=False, twice=False):
    if pos.requires_grad and torch.is_grad_enabled():
        if twice:
            if use_torsion:
                raise NotImplementedError("the torsion has no second-order backward")
            return TripletGeom2Fn.apply(pos, edge_index, num_nodes, mode)
        return TripletGeomFn.apply(pos, edge_index, num_nodes, mode, use_torsion)
    return _run(pos, edge_index, num_nodes, mode, True, use_torsion, True)


def xyz_to_dat(pos, edge_index, num_nodes, use_torsion=False, *, shift=None, shift_idx=None):
    """spherenet_layer.py:496: -> dist, angle, [torsion,] i, j, idx_kj, idx_ji (edge e = j -> i;
    angle in [0, pi] at j; torsion in (0, 2*pi]).  dist, angle and torsion are differentiable
    w.r.t. pos.

    Periodic graphs (K11p, the contract of include/gmp.h): shift (E, 3), the Cartesian shift of
    each edge's image (graph.edge_shift), and shift_idx (E, 3), its integer triple, are given
    together.  The triplets are image-aware, the torsion's candidates are the triplets of the
    same edge, and dist, angle and torsion are functions of the edge vectors
    (pos[j] - pos[i]) + shift, once differentiable in pos and shift (so in the cell)."""
    if (shift is None) != (shift_idx is None):
        raise ValueError("xyz_to_dat: shift and shift_idx are given together")
    if shift_idx is not None:
        vec = edge_vectors(pos, edge_index, shift)
        dist, angle, torsion, idx_kj, idx_ji = _dat_pbc(vec, edge_index, num_nodes, shift_idx,
                                                        use_torsion)
    else:
        dist, angle, torsion, idx_kj, idx_ji = _geom(pos, edge_index, num_nodes, 0, use_torsion)
    j, i = edge_index
    if use_torsion:
        return dist, angle, torsion, i, j, idx_kj, idx_ji
    return dist, angle, i, j, idx_kj, idx_ji


def dimenet_triplets(edge_index, num_nodes, shift_idx=None):
    """PyG DimeNet.triplets as called at dimenet.py:79:
    -> col, row, idx_i, idx_j, idx_k, idx_kj, idx_ji.  With shift_idx (E, 3) the image-aware
    triplets of a periodic graph (K11p: only the reverse image of an edge is left out)."""
    if shift_idx is not None:
        _, _, idx_kj, idx_ji = _run_pbc(None, edge_index, num_nodes, shift_idx)
    else:
        _, _, _, idx_kj, idx_ji = _run(None, edge_index, num_nodes, 1, False, False, False)
    row, col = edge_index
    return col, row, col[idx_ji], row[idx_ji], row[idx_kj], idx_kj, idx_ji


def dimenet_angles(pos, edge_index, num_nodes, twice_differentiable=False, shift=None,
                   shift_idx=None):
    """dimenet.py:79-90: -> dist (E), angle (T, vertex i), i, j, idx_i, idx_j, idx_k, idx_kj,
    idx_ji.  With twice_differentiable the backward to pos is recorded (TripletGeom2Fn), so a
    force can be differentiated again.

    Periodic graphs (K11p, the contract of include/gmp.h): shift (E, 3), the Cartesian shift of
    each edge's image (graph.edge_shift), and shift_idx (E, 3), its integer triple, are given
    together.  The triplets are image-aware, dist and angle are functions of the edge vectors
    (pos[j] - pos[i]) + shift and differentiable in pos and shift (so in the cell)."""
    if (shift is None) != (shift_idx is None):
        raise ValueError("dimenet_angles: shift and shift_idx are given together")
    if shift_idx is not None:
        vec = edge_vectors(pos, edge_index, shift)
        dist, angle, idx_kj, idx_ji = _geom_pbc(vec, edge_index, num_nodes, shift_idx,
                                                twice=twice_differentiable)
    else:
        dist, angle, _, idx_kj, idx_ji = _geom(pos, edge_index, num_nodes, 1,
                                               twice=twice_differentiable)
    row, col = edge_index
    return (dist, angle, col, row, col[idx_ji], row[idx_ji], row[idx_kj], idx_kj, idx_ji)


def xyz_to_dat_offsets(pos, edge_index, num_nodes, *, shift=None, shift_idx=None):
    """xyz_to_dat(..., use_torsion=True) plus the triplet row pointer: -> dist, angle, torsion,
    i, j, idx_kj, idx_ji, offsets (E + 1), the triplets of edge e being the contiguous range
    [offsets[e], offsets[e+1]) (idx_ji is non-decreasing).  shift / shift_idx as xyz_to_dat."""
    dist, angle, torsion, i, j, idx_kj, idx_ji = xyz_to_dat(pos, edge_index, num_nodes, True,
                                                            shift=shift, shift_idx=shift_idx)
    return dist, angle, torsion, i, j, idx_kj, idx_ji, triplet_offsets(idx_ji, dist.numel())


def triplet_offsets(idx_ji, num_edges):
    """Row pointer (E + 1) over the non-decreasing idx_ji (cached per graph)."""
    if num_edges == 0 or idx_ji.numel() == 0:
        return torch.zeros(num_edges + 1, dtype=torch.int64, device=idx_ji.device)
    return ops.get_csr(idx_ji, num_edges).rowptr
