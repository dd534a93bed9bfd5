"""Graph inputs: a PyG-`Batch`-like container, PyG collation, and the synthetic benchmark graphs
(SURVEY.md §8(d)): random 3-D radius graphs with ~1M directed edges, and the k-chains pair
(experiments/kchains.ipynb:71, config C1).

The radius-graph builder is host-side input synthesis (scipy cKDTree), not part of the timed
hot path; a device-side builder is SURVEY.md §8(f) row f1.
"""
import math

import numpy as np
import torch


class Batch:
    """Minimal stand-in for torch_geometric.data.Batch: atoms, pos, edge_index, batch.
    A periodic structure also carries cell (B, 3, 3) (rows = lattice vectors), pbc (three
    booleans) and edge_shift_idx (E, 3) int32, as radius_graph_pbc_gpu returns it."""

    def __init__(self, atoms, pos, edge_index, batch=None, num_graphs=None, cell=None, pbc=None,
                 edge_shift_idx=None, **extra):
        self.atoms = atoms
        self.pos = pos
        self.edge_index = edge_index
        self.batch = batch if batch is not None else torch.zeros(pos.shape[0], dtype=torch.long,
                                                                 device=pos.device)
        self.num_graphs = num_graphs
        self.cell = cell
        self.pbc = pbc
        self.edge_shift_idx = edge_shift_idx
        self.__dict__.update(extra)

    @property
    def num_nodes(self):
        return self.pos.shape[0]

    @property
    def num_edges(self):
        return self.edge_index.shape[1]

    def to(self, device, non_blocking=False):
        kw = {}
        for k, v in self.__dict__.items():
            kw[k] = v.to(device, non_blocking=non_blocking) if torch.is_tensor(v) else v
        return Batch(**kw)


def collate(graphs):
    """PyG Batch.from_data_list semantics: concat nodes, offset edge_index, batch vector.  When
    every graph carries cell, pbc and edge_shift_idx, the cells are stacked to (B, 3, 3), the
    shift indices concatenated and pbc (which all graphs must share) kept."""
    atoms, pos, ei, bv, off = [], [], [], [], 0
    for b, g in enumerate(graphs):
        n = g.pos.shape[0]
        atoms.append(g.atoms)
        pos.append(g.pos)
        ei.append(g.edge_index + off)
        bv.append(torch.full((n,), b, dtype=torch.long))
        off += n
    extra = {}
    if graphs and all(getattr(g, "cell", None) is not None and getattr(g, "pbc", None) is not None
                      and getattr(g, "edge_shift_idx", None) is not None for g in graphs):
        pbc = tuple(bool(v) for v in graphs[0].pbc)
        if any(tuple(bool(v) for v in g.pbc) != pbc for g in graphs):
            raise ValueError("collate: all graphs of a batch share one pbc")
        extra = dict(cell=torch.cat([g.cell.reshape(1, 3, 3) for g in graphs]), pbc=pbc,
                     edge_shift_idx=torch.cat([g.edge_shift_idx for g in graphs]))
    return Batch(torch.cat(atoms), torch.cat(pos), torch.cat(ei, 1), torch.cat(bv),
                 num_graphs=len(graphs), **extra)


def edge_shift(batch):
    """Cartesian shift (E, 3) of each edge's periodic image, from batch.edge_shift_idx and
    batch.cell (differentiable in the cell); None for a batch without images.  The graph of
    each edge is computed once per batch and kept on it as batch.edge_graph."""
    sidx = getattr(batch, "edge_shift_idx", None)
    if sidx is None:
        return None
    cell = getattr(batch, "cell", None)
    if cell is None:
        raise ValueError("batch.edge_shift_idx needs batch.cell")
    from . import ops
    if getattr(batch, "edge_graph", None) is None:
        batch.edge_graph = batch.batch[batch.edge_index[1]]
    return ops.edge_shift_vectors(sidx, cell.reshape(-1, 3, 3), batch.edge_graph)


def radius_edges(pos, r):
    """All ordered pairs a != b with |pos_a - pos_b| < r, as (2, E) int64 sorted by (ei[1], ei[0])."""
    from scipy.spatial import cKDTree

    p = np.asarray(pos, dtype=np.float64)
    pairs = cKDTree(p).query_pairs(r, output_type="ndarray")  # a < b, |pa - pb| <= r
    if pairs.size:
        d = np.linalg.norm(p[pairs[:, 0]] - p[pairs[:, 1]], axis=1)
        pairs = pairs[d < r]
    src = np.concatenate([pairs[:, 0], pairs[:, 1]])
    dst = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.lexsort((src, dst))
    return np.stack([src[order], dst[order]]).astype(np.int64)


def _expected_edges(n, box, r):
    # ignoring boundary effects: n(n-1) * (4/3 pi r^3) / box^3
    return n * (n - 1) * (4.0 / 3.0 * math.pi * r ** 3) / box ** 3


def radius_graph(num_nodes=50_000, target_edges=1_000_000, r=5.0, seed=0, tol=0.01,
                 box=None, shuffle=False):
    """Seeded random radius graph: pos ~ U[0, L)^3 fp32, L tuned by bisection
    so that E is within `tol` of `target_edges` (exact E is whatever the graph has).
    Returns a Batch on CPU (atoms = 0, batch = 0)."""
    rng = np.random.default_rng(seed)
    unit = rng.random((num_nodes, 3))
    if box is None:
        lo, hi = None, None
        box = (num_nodes * num_nodes * 4.0 / 3.0 * math.pi * r ** 3 / target_edges) ** (1 / 3)
        for _ in range(40):
            pos = (unit * box).astype(np.float32)
            ei = radius_edges(pos, r)
            e = ei.shape[1]
            if abs(e - target_edges) <= tol * target_edges:
                break
            if e > target_edges:
                lo = box
            else:
                hi = box
            if lo is not None and hi is not None:
                box = 0.5 * (lo + hi)
            else:
                box = box * (e / target_edges) ** (1 / 3)
    else:
        pos = (unit * box).astype(np.float32)
        ei = radius_edges(pos, r)
    if shuffle:
        ei = ei[:, rng.permutation(ei.shape[1])]
    pos_t = torch.from_numpy(pos)
    return Batch(torch.zeros(num_nodes, dtype=torch.long), pos_t,
                 torch.from_numpy(np.ascontiguousarray(ei)), num_graphs=1, box=float(box),
                 radius=float(r), seed=int(seed))


def create_kchains(k=4):
    """experiments/kchains.ipynb:71: two graphs of k+2 nodes differing in one end position."""
    graphs = []
    for sign in (-1.0, 1.0):
        pos = torch.tensor([[4.0 * sign, -3.0, 0.0]] + [[0.0, 5.0 * i, 0.0] for i in range(k)]
                           + [[4.0, 5.0 * (k - 1) + 3.0, 0.0]])
        pos = pos - pos.mean(0)
        a = torch.arange(k + 1)
        ei = torch.cat([torch.stack([a, a + 1]), torch.stack([a + 1, a])], 1)
        ei = ei[:, torch.argsort(ei[0] * (k + 2) + ei[1])]  # to_undirected sorts by (row, col)
        graphs.append(Batch(torch.zeros(k + 2, dtype=torch.long), pos, ei))
    return graphs


def radius_graph_gpu(pos, r, batch=None, max_num_neighbors=32, num_graphs=None):
    """Device radius graph (K9, gmp_radius_*), the builder PyG SchNet constructs
    (models/schnet.py:47: torch_cluster.radius_graph(pos, r, batch, loop=False,
    max_num_neighbors)).  Edge j -> i for j != i of the same graph with
    ((dx*dx + dy*dy) + dz*dz) < r*r in fp32; per target the first max_num_neighbors + 1
    candidates in ascending j (self included) are kept and self is dropped — torch_cluster's
    GPU selection rule; max_num_neighbors=None or <= 0 keeps all.  Returns edge_index (2, E)
    int64 [sources; targets] sorted by (target, source).  pos: (N, 3) fp32 on the GPU.
    Host syncs: the bounding box, num_graphs (if not given) and the edge count."""
    import ctypes
    from . import _lib, ops
    lib = _lib.load()
    pos = ops._f32c(pos)
    ops._need_cuda(pos)
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must be (N, 3), got {tuple(pos.shape)}")
    if not r > 0:
        raise ValueError("r must be > 0")
    N = pos.shape[0]
    dev = pos.device
    if N == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=dev)
    if batch is not None:
        batch = ops._i64c(batch)
        ops._need_cuda(batch)
        if num_graphs is None:
            num_graphs = int(batch.max().item()) + 1
    num_graphs = 1 if batch is None else int(num_graphs)
    k = 0 if max_num_neighbors is None else max(int(max_num_neighbors), 0)
    lo = pos.min(0).values.cpu().numpy().astype(np.float32)
    hi = pos.max(0).values.cpu().numpy().astype(np.float32)
    r32 = np.float32(r)
    width = float(r32) * (1.0 + 1e-5)  # cell edge > r: rounding in the cell index stays safe
    while True:  # bound the cell table at ~2 cells per node
        inv = float(np.float32(1.0) / np.float32(width))
        if inv > float(np.float32(1.0) / r32):
            width *= 1.0 + 1e-5
            continue
        dims = [max(1, int(np.floor(float(hi[d] - lo[d]) * inv)) + 1) for d in range(3)]
        n_cells = num_graphs * dims[0] * dims[1] * dims[2]
        if n_cells <= 2 * N + 64:
            break
        width *= 1.25
    lo_c = (ctypes.c_float * 3)(*lo.tolist())
    dims_c = (ctypes.c_int * 3)(*dims)
    s = ops._stream()
    cells = torch.empty(N, dtype=torch.int64, device=dev)
    ops.check(lib.gmp_radius_cells_f32(ops._p(pos), ops._p(batch), N, lo_c, inv, dims_c,
                                       ops._p(cells), s), "gmp_radius_cells_f32")
    csr = ops.CSR(cells, n_cells)
    counts = torch.empty(N, dtype=torch.int64, device=dev)
    ops.check(lib.gmp_radius_count_f32(ops._p(pos), ops._p(batch), N, float(r32), k, lo_c, inv,
                                       dims_c, ops._p(cells), ops._p(csr.rowptr),
                                       ops._p(csr.perm), ops._p(counts), s),
              "gmp_radius_count_f32")
    offs = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offs[1:])
    E = int(offs[-1].item())
    src = torch.empty(E, dtype=torch.int64, device=dev)
    if E == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=dev)
    ops.check(lib.gmp_radius_fill_f32(ops._p(pos), ops._p(batch), N, float(r32), k, lo_c, inv,
                                      dims_c, ops._p(cells), ops._p(csr.rowptr),
                                      ops._p(csr.perm), ops._p(offs), ops._p(src), s),
              "gmp_radius_fill_f32")
    dst = torch.repeat_interleave(torch.arange(N, device=dev), counts, output_size=E)
    return torch.stack([src, dst])


# ------------------------------------------------------------------ periodic radius graph (K9p)
PBC_EPS = 1e-3            # bin margin: a bin is at least r (1 + PBC_EPS) wide
PBC_MAX_SHIFT = 127       # |S_k| packs into 8 bits of the sort key
_PBC_ROUND = 12 * 2.0 ** -24  # fp32 error of a bin coordinate per unit of A_k scale_k


def pbc_grid_plan(cell, pbc, r, counts=None, frac_lo=None, frac_hi=None, pos_absmax=None):
    """Host-side grid plan of the periodic radius graph (pure numpy, fp64; the contract is in
    include/gmp.h, the margin argument in csrc/gmp_radius_pbc.hip).

    cell (B, 3, 3), rows = lattice vectors; pbc three booleans; r the cutoff.  Per graph, all
    optional: counts (B) nodes, frac_lo / frac_hi (B, 3) bounds of the fractional coordinates,
    pos_absmax (B, 3) bounds of |pos|.  Returns a dict of arrays: volume (B), heights (B, 3)
    (h_k = V / |a_i x a_j|), nb (B, 3) bins, m (B, 3) reach, inv (B, 3, 3), org / scale (B, 3)
    (bin coordinate = (frac - org) * scale, org = floor(frac) on a periodic axis), base (B + 1)
    first bin of each graph.  Raises ValueError for a cell of the wrong shape or singular,
    r <= 0, a reach, wrap or shift beyond 127, or coordinates too large for the fp32 margin."""
    cell = np.asarray(cell, dtype=np.float64)
    if cell.ndim != 3 or cell.shape[1:] != (3, 3) or cell.shape[0] < 1:
        raise ValueError(f"cell must be (B, 3, 3), got {cell.shape}")
    if not (np.isfinite(r) and r > 0):
        raise ValueError("r must be > 0")
    pbc = tuple(bool(v) for v in pbc)
    if len(pbc) != 3:
        raise ValueError("pbc must hold three booleans")
    B = cell.shape[0]
    per = np.array(pbc)
    counts = np.ones(B, np.int64) if counts is None else np.asarray(counts, np.int64)
    frac_lo = np.zeros((B, 3)) if frac_lo is None else np.asarray(frac_lo, np.float64)
    frac_hi = np.ones((B, 3)) if frac_hi is None else np.asarray(frac_hi, np.float64)
    rr = float(r) * (1.0 + PBC_EPS)
    vol = np.abs(np.linalg.det(cell))
    norms = np.linalg.norm(cell, axis=2)
    if not np.all(np.isfinite(cell)) or np.any(vol <= 1e-9 * np.prod(norms, axis=1)):
        raise ValueError("singular cell")
    cross = np.stack([np.cross(cell[:, 1], cell[:, 2]), np.cross(cell[:, 2], cell[:, 0]),
                      np.cross(cell[:, 0], cell[:, 1])], 1)
    heights = vol[:, None] / np.linalg.norm(cross, axis=2)
    inv = np.linalg.inv(cell)
    if not (np.all(np.isfinite(frac_lo)) and np.all(np.isfinite(frac_hi))):
        raise ValueError("pos is not finite")
    extent = np.maximum(frac_hi - frac_lo, 0.0)
    width = np.where(per, heights, extent * heights)  # perpendicular width to divide into bins
    nb = np.maximum(1, np.floor(width / rr)).astype(np.int64)
    for b in range(B):  # bound the bin table at ~2 bins per node, as K9 does
        while nb[b].prod() > 2 * max(int(counts[b]), 0) + 8:
            nb[b] = np.maximum(1, np.floor(nb[b] * 0.8)).astype(np.int64)
    m = np.where(per, np.ceil(rr * nb / heights), (nb > 1).astype(np.float64)).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(per, nb.astype(np.float64), np.where(nb > 1, nb / extent, 0.0))
    org = np.where(per, 0.0, frac_lo)
    if m.max() > PBC_MAX_SHIFT:
        raise ValueError(f"the cutoff reaches {int(m.max())} bins of a cell thinner than r: "
                         f"more than {PBC_MAX_SHIFT} images along one axis are not supported")
    w_lo, w_hi = np.floor(frac_lo) - 1, np.floor(frac_hi) + 1  # one spare for fp32 rounding
    q_max = -(-m // nb)
    wraps = np.where(per, np.maximum(np.abs(w_lo), np.abs(w_hi)), 0)
    shifts = np.where(per, q_max + (w_hi - w_lo), 0)
    if max(wraps.max(), shifts.max()) > PBC_MAX_SHIFT:
        raise ValueError(f"atoms lie more than {PBC_MAX_SHIFT} cells apart or away from the "
                         "origin: wrap them closer to the cell")
    if pos_absmax is not None:
        A = np.maximum(1.0, np.einsum("bd,bdk->bk", np.asarray(pos_absmax, np.float64),
                                      np.abs(inv)))
        if np.any(2 * _PBC_ROUND * A * scale > PBC_EPS / (1 + PBC_EPS)):
            raise ValueError("fractional coordinates too large for the fp32 bin margin "
                             "(|frac| * bins per axis beyond ~700): wrap the atoms closer to "
                             "the cell")
    base = np.zeros(B + 1, np.int64)
    np.cumsum(nb.prod(1), out=base[1:])
    return dict(volume=vol, heights=heights, nb=nb, m=m, inv=inv, org=org, scale=scale,
                base=base, pbc=pbc)


def radius_graph_pbc_gpu(pos, r, cell, pbc=(True, True, True), batch=None, num_graphs=None):
    """Device radius graph under periodic boundary conditions (K9p, gmp_radius_pbc_*; the
    contract is stated in include/gmp.h).  pos (N, 3) fp32 on the GPU, cell (B, 3, 3) (or (3, 3)
    for one graph) with rows = lattice vectors, pbc three booleans shared by all graphs.
    Returns (edge_index (2, E) int64 [sources; targets], edge_shift_idx (E, 3) int32), sorted by
    (target, source, S0, S1, S2); no neighbour cap.  Host syncs: the cell, the per-graph bounds
    of the fractional coordinates, and the edge count."""
    from . import _lib, ops
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must be (N, 3), got {tuple(pos.shape)}")
    if not r > 0:
        raise ValueError("r must be > 0")
    N, dev = pos.shape[0], pos.device
    cell_h = torch.as_tensor(cell).detach().to("cpu", torch.float32)
    if cell_h.dim() == 2:
        cell_h = cell_h.unsqueeze(0)
    if cell_h.dim() != 3 or tuple(cell_h.shape[1:]) != (3, 3):
        raise ValueError(f"cell must be (B, 3, 3), got {tuple(cell_h.shape)}")
    if batch is not None and num_graphs is None:
        num_graphs = int(batch.max().item()) + 1 if N else cell_h.shape[0]
    B = 1 if batch is None else int(num_graphs)
    if cell_h.shape[0] != B:
        raise ValueError(f"one cell per graph: got {cell_h.shape[0]} cells for {B} graphs")
    cell64 = cell_h.numpy().astype(np.float64)  # the one copy every plan quantity comes from
    plan = pbc_grid_plan(cell64, pbc, float(np.float32(r)))  # singular cell, reach of r
    lib = _lib.load()
    pos = ops._f32c(pos)
    ops._need_cuda(pos)
    if batch is not None:
        batch = ops._i64c(batch)
        ops._need_cuda(batch)
    empty = (torch.empty((2, 0), dtype=torch.int64, device=dev),
             torch.empty((0, 3), dtype=torch.int32, device=dev))
    if N == 0:
        return empty
    # per-graph bounds of frac, -frac and |pos|, and the node counts: one sync
    inv32 = torch.from_numpy(plan["inv"].astype(np.float32)).to(dev)
    if batch is None:
        frac = (pos.unsqueeze(2) * inv32[0]).sum(1)
        vals = torch.cat([frac, -frac, pos.abs()], 1)
        stats = torch.cat([vals.amax(0), vals.new_tensor([float(N)])]).view(1, 10)
    else:  # the deterministic segmented max over the CSR of batch (empty graphs: zeros)
        frac = (pos.unsqueeze(2) * inv32[batch.clamp(0, B - 1)]).sum(1)
        bcsr = ops.get_csr(batch, B)
        smax, _ = ops.segment_reduce(torch.cat([frac, -frac, pos.abs()], 1), bcsr, "max")
        stats = torch.cat([smax, bcsr.counts().to(torch.float32).view(B, 1)], 1)
    st = stats.cpu().numpy().astype(np.float64)
    plan = pbc_grid_plan(cell64, pbc, float(np.float32(r)), counts=st[:, 9].astype(np.int64),
                         frac_lo=-st[:, 3:6], frac_hi=st[:, 0:3], pos_absmax=st[:, 6:9])
    gi = np.zeros((B, 8), np.int32)
    gi[:, 0:3], gi[:, 3:6] = plan["nb"], plan["m"]
    gi[:, 6] = sum(1 << k for k in range(3) if plan["pbc"][k])
    gf = np.concatenate([plan["inv"].reshape(B, 9), plan["org"], plan["scale"],
                         cell64.reshape(B, 9)], 1).astype(np.float32)
    n_bins = int(plan["base"][-1])
    gi_d, gf_d = torch.from_numpy(gi).to(dev), torch.from_numpy(gf).to(dev)
    gb_d = torch.from_numpy(plan["base"][:-1].copy()).to(dev)
    s = ops._stream()
    r32 = float(np.float32(r))
    bins = torch.empty(N, dtype=torch.int64, device=dev)
    wraps = torch.empty(N, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    common = (ops._p(pos), ops._p(batch), N, B)
    plan_p = (ops._p(gi_d), ops._p(gf_d), ops._p(gb_d))
    ops.check(lib.gmp_radius_pbc_bins_f32(*common, *plan_p, ops._p(bins), ops._p(wraps),
                                          ops._p(err), s), "gmp_radius_pbc_bins_f32")
    csr = ops.CSR(bins, n_bins)
    counts = torch.empty(N, dtype=torch.int64, device=dev)
    ops.check(lib.gmp_radius_pbc_count_f32(*common, r32, *plan_p, ops._p(bins), ops._p(wraps),
                                           ops._p(csr.rowptr), ops._p(csr.perm),
                                           ops._p(counts), ops._p(err), s),
              "gmp_radius_pbc_count_f32")
    offs = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offs[1:])
    E, bad = (int(v) for v in torch.stack([offs[-1], err[0].to(torch.int64)]).tolist())
    if bad:
        raise ValueError("radius_graph_pbc_gpu: a batch entry outside [0, num_graphs) or a "
                         f"periodic image beyond {PBC_MAX_SHIFT} cells")
    if E == 0:
        return empty
    src = torch.empty(E, dtype=torch.int64, device=dev)
    sidx = torch.empty((E, 3), dtype=torch.int32, device=dev)
    ops.check(lib.gmp_radius_pbc_fill_f32(*common, r32, *plan_p, ops._p(bins), ops._p(wraps),
                                          ops._p(csr.rowptr), ops._p(csr.perm), ops._p(offs),
                                          ops._p(src), ops._p(sidx), ops._p(err), s),
              "gmp_radius_pbc_fill_f32")
    dst = torch.repeat_interleave(torch.arange(N, device=dev), counts, output_size=E)
    return torch.stack([src, dst]), sidx
