"""CPU model of the receivers' sums that four edge kernels do themselves (TEST INFRASTRUCTURE).

egnn_fwd_kernel, egnn_bwd_kernel (csrc/gmp_egnn.hip with csrc/gmp_egnn_common.h),
gvp_layer_fwd_agg_kernel and gvp_msg0_bwd_agg_kernel (csrc/gmp_gvp.hip) share one mechanism,
restated here from their code:

  * node_begin / agg_node_begin: wave w of n_waves starts at the first receiver n in [0, N] with
    rowptr[n] >= (E * w) / n_waves (w <= 0: 0, w >= n_waves: N); a wave owns the receivers
    [nb(w), nb(w + 1)) and their in-edges [rowptr[nb(w)], rowptr[nb(w + 1)]), or no edge when
    the node range is empty;
  * the wave walks its edges in chunks of 16 from its own e_lo; inside a chunk a segmented scan
    sums each receiver's lanes (head = first lane of the lane's segment in the chunk);
  * lane 15 leaves its running sum in an LDS carry after every chunk; lane 0 of the next chunk
    adds it only if its receiver is the receiver lane 15 had (carry_node);
  * a receiver's row is written by the last edge of its segment; rows of in-degree 0 are zeroed
    by a lane-strided loop over the wave's node range, 64 receivers per pass.

wave_ranges and events say which corners of that mechanism a graph reaches at a given wave
count; model_sum is the same walk in fp64 (optionally with one of two deliberate faults); the
bound helpers turn per-edge fp64 terms into per-row error bounds.  Nothing here touches a GPU.
"""
import numpy as np
import torch

CHUNK = 16
FWD_WAVES = 12   # kFwdWaves: waves per workgroup of the EGNN forward
BWD_WAVES = 8    # kBwdWaves: ... of the EGNN backward
GVP_WAVES = 8    # kGT / 64: ... of the two GVP kernels
MIN_CUS = 64     # from here on the counts below do not depend on the device for E <= ~11000
U23 = 2.0 ** -23

SITUATIONS = (
    "carry_2", "carry_ge9", "hub_eats_waves", "end_on_lane15_then_new_segment",
    "full_chunk_one_segment", "sixteen_singletons", "partial_last_chunk",
    "range_shorter_than_chunk", "isolated_run_gt64", "isolated_leading", "isolated_trailing",
    "empty_wave")


# ------------------------------------------------------------------------------- wave counts
def _ceil_div(a, b):
    return -(-a // b)


def egnn_waves(n_edges, cus, nwb):
    """n_waves_for (gmp_egnn.hip): ceil(E / 128) capped at CUs * nwb, at least 1, rounded up to
    whole workgroups of nwb waves."""
    w = min(_ceil_div(n_edges, 128), cus * nwb)
    return _ceil_div(max(w, 1), nwb) * nwb


def egnn_fwd_waves(n_edges, cus):
    return egnn_waves(n_edges, cus, FWD_WAVES)


def egnn_bwd_waves(n_edges, cus):
    return egnn_waves(n_edges, cus, BWD_WAVES)


def gvp_waves(n_edges, cus):
    """gmp_gvp_layer_fwd_agg_f32 / gmp_gvp_msg0_bwd_agg_f32: min(CUs, ceil(E / 512)) workgroups
    (at least one) of 8 waves."""
    return max(min(cus, _ceil_div(n_edges, GVP_WAVES * 64)), 1) * GVP_WAVES


WAVE_COUNTS = {"egnn_fwd": egnn_fwd_waves, "egnn_bwd": egnn_bwd_waves, "gvp": gvp_waves}


# ------------------------------------------------------------------------------- the split
def rowptr_of(recv, n_nodes):
    """int64 numpy rowptr (N + 1) of the receivers' CSR."""
    deg = np.bincount(np.asarray(recv, dtype=np.int64), minlength=n_nodes)
    assert deg.shape[0] == n_nodes
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)


def node_begin(rowptr, w, n_waves):
    n, e = len(rowptr) - 1, int(rowptr[-1])
    if w >= n_waves:
        return n
    if w <= 0:
        return 0
    target = (e * w) // n_waves
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) >> 1
        if rowptr[mid] < target:
            lo = mid + 1
        else:
            hi = mid
    return lo


def wave_ranges(rowptr, n_waves):
    """[(n_lo, n_hi, e_lo, e_hi)] per wave (wave_range in gmp_egnn_common.h; the GVP kernels'
    nb / ne / e_lo / e_hi)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nb = [node_begin(rowptr, w, n_waves) for w in range(n_waves + 1)]
    out = []
    for w in range(n_waves):
        lo, hi = nb[w], nb[w + 1]
        out.append((lo, hi, int(rowptr[lo]), int(rowptr[hi])) if lo < hi else (lo, hi, 0, 0))
    return out


def events(rowptr, n_waves):
    """The set of SITUATIONS that the walk of `n_waves` waves over this CSR meets."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    deg = rowptr[1:] - rowptr[:-1]
    recv = np.repeat(np.arange(n), deg)  # receiver of sorted edge k
    ev = set()
    if n and deg[0] == 0:
        ev.add("isolated_leading")
    if n and deg[-1] == 0:
        ev.add("isolated_trailing")
    ranges = wave_ranges(rowptr, n_waves)
    eaten, eaten_at = 0, None
    for (n_lo, n_hi, e_lo, e_hi) in ranges:
        if n_lo == n_hi:
            ev.add("empty_wave")
            # an empty wave that starts at receiver n_lo >= 1: its own target and the next
            # wave's both lie inside the segment of receiver n_lo - 1 (node_begin's search)
            eaten = eaten + 1 if (n_lo >= 1 and eaten_at == n_lo) else (1 if n_lo >= 1 else 0)
            eaten_at = n_lo
            if eaten >= 3:
                ev.add("hub_eats_waves")
            continue
        eaten, eaten_at = 0, None
        run = 0
        for d in deg[n_lo:n_hi]:
            run = run + 1 if d == 0 else 0
            if run >= 65:
                ev.add("isolated_run_gt64")
        if 0 < e_hi - e_lo < CHUNK:
            ev.add("range_shorter_than_chunk")
        for node in range(n_lo, n_hi):
            if deg[node] == 0:
                continue
            s0, s1 = int(rowptr[node]), int(rowptr[node + 1])
            span = (s1 - 1 - e_lo) // CHUNK - (s0 - e_lo) // CHUNK + 1
            if span == 2:
                ev.add("carry_2")
            if span >= 9:
                ev.add("carry_ge9")
            if deg[node] == CHUNK and (s0 - e_lo) % CHUNK == 0:
                ev.add("full_chunk_one_segment")
        for base in range(e_lo, e_hi, CHUNK):
            ne = min(CHUNK, e_hi - base)
            # (after a wave's first chunk the carry slot holds lane 15's sum: not zero)
            if base > e_lo and recv[base] != recv[base - 1]:
                ev.add("end_on_lane15_then_new_segment")
            if ne == CHUNK and bool((deg[recv[base:base + CHUNK]] == 1).all()):
                ev.add("sixteen_singletons")
            # the segment of the last valid lane came in through the carry (seg0 < base)
            if ne < CHUNK and rowptr[recv[base + ne - 1]] < base:
                ev.add("partial_last_chunk")
    return ev


# ------------------------------------------------------------------------------- the walk in fp64
def sorted_edges(recv, n_nodes):
    """(perm, rowptr): the stable receiver sort gmp_csr_build makes."""
    recv = torch.as_tensor(recv, dtype=torch.int64)
    perm = torch.argsort(recv, stable=True)
    return perm, rowptr_of(recv.numpy(), n_nodes)


def model_sum(terms, recv, n_nodes, n_waves, fault=None):
    """The kernels' walk over fp64 per-edge `terms` (E, F) in input order: (N, F) receiver sums.
    fault = "drop_first_chunk": lane 0 does not take the carry of a segment whose first chunk
    was the previous one (that chunk's contribution is lost); fault = "spurious_carry": lane 0
    takes the stale carry although its receiver differs from carry_node.  Returns (sums, hits):
    hits = how many times the fault was applied."""
    assert fault in (None, "drop_first_chunk", "spurious_carry")
    perm, rowptr = sorted_edges(recv, n_nodes)
    t = terms.double()[perm]
    recv_s = np.asarray(recv)[perm.numpy()]
    out = torch.zeros(n_nodes, t.shape[1], dtype=torch.float64)
    hits = 0
    for (n_lo, n_hi, e_lo, e_hi) in wave_ranges(rowptr, n_waves):
        carry, carry_node = torch.zeros(t.shape[1], dtype=torch.float64), -1
        for base in range(e_lo, e_hi, CHUNK):
            ne = min(CHUNK, e_hi - base)
            x = t[base:base + ne].clone()
            take = recv_s[base] == carry_node
            if fault == "spurious_carry" and not take and base > e_lo:
                take, hits = True, hits + 1
            if fault == "drop_first_chunk" and take and rowptr[recv_s[base]] >= base - CHUNK:
                take, hits = False, hits + 1
            if take:
                x[0] += carry
            for lane in range(ne):
                node = recv_s[base + lane]
                if lane > 0 and recv_s[base + lane - 1] == node:
                    x[lane] += x[lane - 1]
                if base + lane == rowptr[node + 1] - 1:
                    out[node] = x[lane]
            if ne == CHUNK:
                carry, carry_node = x[CHUNK - 1].clone(), recv_s[base + CHUNK - 1]
    return out, hits


# ------------------------------------------------------------------------------- bounds
def degrees(recv, n_nodes):
    return torch.bincount(torch.as_tensor(recv, dtype=torch.int64), minlength=n_nodes)


def index_sum(terms, recv, n_nodes):
    """fp64 index_add_ of per-edge rows (E, ...) at the receivers: (N, ...)."""
    t = terms.double()
    return torch.zeros((n_nodes,) + t.shape[1:], dtype=torch.float64).index_add_(
        0, torch.as_tensor(recv, dtype=torch.int64), t)


def sum_bound(terms, recv, n_nodes, mean=False, extra=16):
    """(ref, bound) of an fp32 sum, in any order, of the fp32 per-edge rows `terms` at the
    receivers: |got - ref| <= (deg + extra) 2^-23 sum |t| per row and component (the standard
    (n - 1) u sum |t| with u = 2^-24 and a factor of two in hand; extra = 16 covers the carry
    adds and, at 18, one rounding of a product formed on the way).  mean: both divided by the
    degree (isolated rows: 0) and 2^-23 |ref| added for the division."""
    deg = degrees(recv, n_nodes).double()
    shape = (n_nodes,) + (1,) * (terms.dim() - 1)
    ref = index_sum(terms, recv, n_nodes)
    bound = (deg.view(shape) + extra) * U23 * index_sum(terms.double().abs(), recv, n_nodes)
    if mean:
        d = deg.clamp(min=1).view(shape)
        ref = ref / d
        bound = bound / d + U23 * ref.abs()
    return ref, bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries with a positive bound; inf if an entry with a
    zero bound differs from its reference."""
    err = (got.double() - ref).abs()
    if bool((err[bound == 0] != 0).any()):
        return float("inf")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def assert_within(got, ref, bound, name):
    """got (fp32 or fp64) within the per-entry bound of ref; prints the worst ratio first."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    r = worst_ratio(got.detach().cpu(), ref, bound)
    print(f"{name}: worst |got - ref| / bound = {r:.3g}")
    assert r <= 1.0, f"{name}: |got - ref| reaches {r:.3g} x its bound"
    return r


def assert_zero_rows(got, recv, n_nodes, name):
    """Rows of receivers without in-edges are +0 in every component."""
    rows = got.detach().cpu()[degrees(recv, n_nodes) == 0]
    assert not bool((rows != 0).any()) and not bool(torch.signbit(rows).any()), name


def row_scale_bound(edge_rows, recv, n_nodes, factor, mean):
    """The EGNN feature bar per row: factor * A_n, A_n = sum over the in-edges of max_f |row|
    in fp64 (divided by the degree for a mean): (N, 1)."""
    a = index_sum(edge_rows.double().abs().amax(dim=1, keepdim=True), recv, n_nodes)
    if mean:
        a = a / degrees(recv, n_nodes).clamp(min=1).double().view(-1, 1)
    return factor * a


def grad_row_bound(ref, factor):
    """The EGNN gradient bar per row: factor * (|ref_n|_inf + median_n |ref_n|_inf): (N, 1)."""
    rn = ref.abs().amax(dim=1, keepdim=True)
    return factor * (rn + rn.median())


def gvp_row_variation(s, v, W):
    """(ds (E, 128), dv (E, 48)) in fp64: how far two fp32 evaluations of one (128, 16) ->
    (128, 16) GVP's per-edge rows may lie apart when they differ only in how the compiler
    contracted |vh|^2 = x^2 + y^2 + z^2 (gvp_layer_fwd_x3_kernel forms fma(z, z, fma(y, y, x x)),
    gvp_layer_fwd_agg_kernel a packed multiply, one fma and an add: read from the two kernels'
    code objects), every product running on the same MFMA chain.  With u = 2^-24:
      |vh|^2 is a sum of three positive terms, each form within 3u of it, and sqrtf is correctly
        rounded: the two vn differ by at most (3u + 2u) vn, taken as 6u vn;
      spre = bs + Ws[:, :128] s (the same bits in both) + Ws[:, 128:] vn in 4 MFMA steps of 4
        products; a step is taken to err by at most 8u of the magnitudes it adds, so with
        M_f = |bs_f| + sum |Ws_fk| |s_k| + sum |Ws_f,128+k| vn_k each evaluation is within 32u M_f
        of its exact value, and the exact values differ by at most 6u M_f: ds = 70u M;
      gate = bsv + Wsv spre in 32 such steps: dgate = |Wsv| ds + 2 x 32 x 8u Mg, Mg = |bsv| +
        |Wsv| M;
      sigmoid' <= 1/4, and 1 / (1 + __expf(-x)) is within (|x| + 4)u of the sigmoid (the
        exponent's scaling rounds at |x| u, v_exp_f32 and the division at one unit each):
        dsg = dgate / 4 + 2 (|gate| + 4) u; v_out = vpre sg is one rounding of the same vpre:
        dv = |vpre| (dsg + 2u).
    Derived from the inputs alone and generous; tests/test_segsum_host.py shows that a dropped or
    a stale carry still falls far outside the bound with it added.
    What it costs: on v the gate's term 512u Mg / 4 comes to about 2e-4 of a per-edge row, some
    100 x the summation bound and above the project's 1e-5 feature bar, so on v_agg the fused
    forward test catches a missing or a foreign contribution but not an error of a few 1e-5
    relative (s_agg, at 70u M, stays near the summation bound).  A tighter allowance would carry
    only vn's 6u through the two identical MFMA chains; pinning vnorm's contraction in the two
    kernels would make the rows bitwise again and remove the allowance altogether."""
    Ws, bs, Wsv, bsv, Wh, Wv = (t.detach().cpu().double() for t in W)
    s, v = s.detach().cpu().double(), v.detach().cpu().double()
    u = 2.0 ** -24
    vh = torch.einsum("hc,ecx->ehx", Wh, v)
    vn = vh.pow(2).sum(-1).clamp(min=1e-8).sqrt()
    M = bs.abs() + s.abs() @ Ws[:, :128].abs().t() + vn @ Ws[:, 128:].abs().t()
    ds = 70 * u * M
    spre = bs + s @ Ws[:, :128].t() + vn @ Ws[:, 128:].t()
    gate = bsv + spre @ Wsv.t()
    dgate = ds @ Wsv.abs().t() + 512 * u * (bsv.abs() + M @ Wsv.abs().t())
    dsg = dgate / 4 + 2 * (gate.abs() + 4) * u
    vpre = torch.einsum("oh,ehx->eox", Wv, vh).abs()
    dv = vpre * (dsg + 2 * u).unsqueeze(-1)
    return ds, dv.reshape(v.shape[0], -1)


# ------------------------------------------------------------------------------- graphs
class Graph:
    """edge_index (2, E) int64 = (senders j, receivers i) in shuffled input order, pos (N, 3)."""

    def __init__(self, name, n, edge_index, pos):
        self.name, self.n, self.edge_index, self.pos = name, n, edge_index, pos
        self.rowptr = rowptr_of(edge_index[1].numpy(), n)

    @property
    def E(self):
        return self.edge_index.shape[1]

    @property
    def recv(self):
        return self.edge_index[1]


def _finish(name, n, send, recv, gen):
    send, recv = torch.as_tensor(send, dtype=torch.int64), torch.as_tensor(recv, dtype=torch.int64)
    assert not bool((send == recv).any())
    order = torch.randperm(send.shape[0], generator=gen)
    ei = torch.stack([send[order], recv[order]]).contiguous()
    pos = torch.rand(n, 3, generator=gen) * 4.0
    return Graph(name, n, ei, pos)


def _senders(recv, n, gen):
    """uniform senders != receiver"""
    s = torch.randint(0, n - 1, recv.shape, generator=gen)
    return s + (s >= recv).long()


# In receiver order.  16 first (after the leading isolated receivers), so that its segment fills
# the first chunk of wave 0 exactly and the 17 that follows meets a stale carry and spans two
# chunks; 2 and 3 are for K13, which keeps two rows in flight; the hub (more than half of E)
# swallows the targets of many waves; 70 isolated receivers in a row sit in one wave's node
# range (every one of them has the same rowptr).
PATTERN_DEGREES = ([0] * 3 + [16, 17, 15, 1, 0, 31, 32, 33, 2, 3] + [1] * 16 + [150] + [0] * 70
                   + [2500] + [1] * 40)
PATTERN_FILLER_NODES, PATTERN_FILLER_EDGES, PATTERN_TAIL = 100, 1500, 5


def patterns(seed=0):
    """The composite graph: the explicit degree list, then 100 receivers sharing 1500
    uniform-random filler edges (a few of them the same (j, i) pair twice), then 5 isolated
    receivers."""
    gen = torch.Generator().manual_seed(seed)
    n0 = len(PATTERN_DEGREES)
    n = n0 + PATTERN_FILLER_NODES + PATTERN_TAIL
    recv = torch.repeat_interleave(torch.arange(n0), torch.tensor(PATTERN_DEGREES))
    fill = n0 + torch.randint(0, PATTERN_FILLER_NODES, (PATTERN_FILLER_EDGES,), generator=gen)
    recv = torch.cat([recv, fill.sort().values])
    send = _senders(recv, n, gen)
    dups = 0
    for k in range(recv.shape[0] - PATTERN_FILLER_EDGES, recv.shape[0] - 1, 97):
        if recv[k] == recv[k + 1]:  # multi-edges among the filler: the pair (j, i) twice
            send[k + 1] = send[k]
            dups += 1
    assert dups >= 3
    g = _finish("patterns", n, send, recv, gen)
    assert g.E % CHUNK != 0 and g.n <= 700 and g.E <= 6000
    return g


def star(n=300):
    """Receiver 0 gets an edge from every other node and sends one to each: a hub on the
    receiver side and on the sender side."""
    gen = torch.Generator().manual_seed(n)
    others = torch.arange(1, n)
    send = torch.cat([others, torch.zeros(n - 1, dtype=torch.int64)])
    recv = torch.cat([torch.zeros(n - 1, dtype=torch.int64), others])
    return _finish("star", n, send, recv, gen)


def tiny(n_edges, n=20):
    """E edges into receiver 3 of 20 nodes, the senders cycling over the other nodes."""
    gen = torch.Generator().manual_seed(n_edges)
    others = [k for k in range(n) if k != 3]
    send = [others[k % len(others)] for k in range(n_edges)]
    return _finish(f"tiny{n_edges}", n, send, [3] * n_edges, gen)


def control():
    """The radius graph the GVP tests use: near-uniform in-degree, one graph."""
    from gmp_amd.graph import radius_graph
    g = radius_graph(num_nodes=600, target_edges=9000, r=2.0, seed=4, tol=0.2, shuffle=True)
    return Graph("control", g.num_nodes, g.edge_index.contiguous(), g.pos)


_GRAPHS = {}


def graph(name):
    """patterns | star | tiny1 | tiny15 | tiny16 | tiny17 | control, built once."""
    if name not in _GRAPHS:
        if name.startswith("tiny"):
            _GRAPHS[name] = tiny(int(name[4:]))
        else:
            _GRAPHS[name] = {"patterns": patterns, "star": star, "control": control}[name]()
    return _GRAPHS[name]


NEW_GRAPHS = ("patterns", "star", "tiny1", "tiny15", "tiny16", "tiny17")
ALL_GRAPHS = NEW_GRAPHS + ("control",)

# What each graph is relied on for, at each of the three wave counts (tests/test_segsum_host.py
# asserts it with 256 CUs, the GPU tests with the launch's own count).  Their union is SITUATIONS.
EXPECT = {
    "patterns": {"carry_2", "carry_ge9", "hub_eats_waves", "end_on_lane15_then_new_segment",
                 "full_chunk_one_segment", "sixteen_singletons", "partial_last_chunk",
                 "isolated_run_gt64",
                 "isolated_leading", "isolated_trailing", "empty_wave"},
    "star": {"carry_ge9", "hub_eats_waves", "sixteen_singletons", "empty_wave",
             "end_on_lane15_then_new_segment", "partial_last_chunk"},
    "tiny1": {"range_shorter_than_chunk", "isolated_leading", "isolated_trailing", "empty_wave"},
    "tiny15": {"range_shorter_than_chunk", "isolated_leading", "isolated_trailing"},
    "tiny16": {"full_chunk_one_segment", "isolated_leading", "isolated_trailing"},
    "tiny17": {"carry_2", "partial_last_chunk", "isolated_leading", "isolated_trailing"},
    "control": set(),
}
CONTROL_LACKS = {"carry_ge9", "hub_eats_waves", "isolated_run_gt64"}


def assert_events(g, n_waves, kernel):
    """The graph reaches, at this launch's wave count, what the tests rely on it for."""
    ev = events(g.rowptr, n_waves)
    missing = EXPECT[g.name] - ev
    assert not missing, f"{kernel}: {g.name} at {n_waves} waves lacks {sorted(missing)}"
    return ev


# ------------------------------------------------------------------------------- EGNN block
def perturbed_oracle_layer(d, act, aggr, seed):
    """oracle.egnn.EGNNLayer with its 1-D parameters moved off their initial values."""
    from oracle import egnn as oegnn
    torch.manual_seed(seed)
    ref = oegnn.EGNNLayer(d, act, "layer", aggr)
    with torch.no_grad():
        for p in ref.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return ref


def egnn_block(layer, h, pos, edge_index, n_nodes):
    """The message block of oracle.egnn.EGNNLayer.forward from the layer's own submodules, in
    the dtype of its arguments, with dim_size = n_nodes (the module's scatter has none, so it
    cannot have trailing isolated receivers): (m_aggr, pos_aggr, m, shift)."""
    j, i = edge_index[0], edge_index[1]
    rel = pos[i] - pos[j]
    dist = rel.norm(dim=-1, keepdim=True)
    m = layer.mlp_msg(torch.cat([h[i], h[j], dist], dim=-1))  # [h_i, h_j, dist]
    shift = rel * layer.mlp_pos(m)
    deg = degrees(i, n_nodes).clamp(min=1).to(m.dtype).view(-1, 1)
    m_aggr = torch.zeros(n_nodes, m.shape[1], dtype=m.dtype).index_add_(0, i, m)
    if layer.aggr == "mean":
        m_aggr = m_aggr / deg
    p_aggr = torch.zeros(n_nodes, 3, dtype=m.dtype).index_add_(0, i, shift) / deg  # always mean
    return m_aggr, p_aggr, m, shift


BLOCK_PARAMS = ("mlp_msg", "mlp_pos")  # the parameters the message block reads


def egnn_block_run(layer, h, pos, edge_index, n_nodes, gm, gp):
    """Forward and backward of egnn_block with the loss sum(m_aggr gm) + sum(pos_aggr gp):
    dict with m_aggr, pos_aggr, m, shift, dh, dpos and grads = {parameter name: gradient}."""
    dt = next(layer.parameters()).dtype
    for p in layer.parameters():
        p.grad = None
    hr = h.detach().to(dt).clone().requires_grad_(True)
    pr = pos.detach().to(dt).clone().requires_grad_(True)
    m_aggr, p_aggr, m, shift = egnn_block(layer, hr, pr, edge_index, n_nodes)
    ((m_aggr * gm.to(dt)).sum() + (p_aggr * gp.to(dt)).sum()).backward()
    grads = {k: p.grad.detach().clone() for k, p in layer.named_parameters()
             if k.startswith(BLOCK_PARAMS)}
    return dict(m_aggr=m_aggr.detach(), pos_aggr=p_aggr.detach(), m=m.detach(),
                shift=shift.detach(), dh=hr.grad, dpos=pr.grad, grads=grads)


def egnn_inputs(g, d, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(g.n, d, generator=gen), torch.randn(g.n, d, generator=gen),
            torch.randn(g.n, 3, generator=gen))


FEATURE_BAR, GRAD_BAR = 1e-5, 1e-4  # the project's feature and gradient bars (BASELINE.json)


def pos_floor(oracle32, ref64, g):
    """(floor, rows): the absolute allowance on the pos_aggr rows of single-edge receivers, and
    the rows on which the fp32 CPU oracle misses 1e-5 A_n.  A per-edge shift is
    rel (w4 . y3 + b4), and the scalar cancels to 1e-3 of its terms on some edges; a receiver
    whose ONE shift is of that kind has an A_n (that shift's own size) far below the fp32
    rounding of the scalar, and the oracle itself misses 1e-5 A_n there (degree-1 rows of `star`
    and `patterns`; DESIGN.md section 5 has example figures).  Which degree-1 rows a given fp32
    order misses is chance, so the floor covers all of them, and only them: such a row is one
    term, no sum, and no carry can feed it.  From two in-edges on the oracle meets the
    bar as it stands (tests/test_segsum_host.py), so every other row keeps exactly 1e-5 A_n
    (egnn_check asserts the confinement).
    floor = 4 x the oracle's largest absolute error over the rows where it misses the bar (HF is
    allowed 2 x the exact path, the exact path 2 x another fp32 order), 0 where it misses none.
    It depends on the CPU's fp32 rounding order, never on a kernel's output."""
    bar = row_scale_bound(ref64["shift"], g.recv, g.n, FEATURE_BAR, True)
    err = (oracle32["pos_aggr"].double() - ref64["pos_aggr"]).abs().amax(dim=1, keepdim=True)
    over = (err > bar).flatten()
    return (4.0 * float(err[over].max()) if bool(over.any()) else 0.0), torch.nonzero(over).flatten()


def egnn_check(got, ref64, g, mean, name, floor=0.0, floor_rows=None):
    """`got` (dict as egnn_block_run's, any float dtype) against the fp64 run `ref64` under the
    per-row bars: 1e-5 A_n on m_aggr and pos_aggr, exact +0 rows for isolated receivers,
    1e-4 (|ref_n|_inf + median_n |ref_n|_inf) on dh and dpos, tests/test_gpu_egnn.py's
    _assert_grads rule on the parameters.  (floor, floor_rows) are pos_floor's: the pos_aggr
    rows of single-edge receivers get max(1e-5 A_n, floor), every other row exactly 1e-5 A_n;
    the rows the oracle misses must all be such receivers, and floor at most the project's
    absolute 1e-5.  Returns the largest absolute error of each output."""
    e = {}
    deg = degrees(g.recv, g.n)
    single = (deg == 1).view(-1, 1)
    if floor:
        assert floor <= FEATURE_BAR, f"{name}: pos_aggr floor {floor:.3g}"
        assert floor_rows is not None and bool((deg[floor_rows] == 1).all()), \
            f"{name}: the oracle misses 1e-5 A_n on receivers of degree {deg[floor_rows].tolist()}"
    for key, rows, mn, fl in (("m_aggr", "m", mean, 0.0), ("pos_aggr", "shift", True, floor)):
        bound = row_scale_bound(ref64[rows], g.recv, g.n, FEATURE_BAR, mn)
        if fl:
            bound = torch.where(single, bound.clamp(min=fl), bound)
        bound = bound * (deg > 0).view(-1, 1)  # isolated rows: exactly zero
        assert_within(got[key], ref64[key], bound.expand_as(ref64[key]), f"{name} {key}")
        assert_zero_rows(got[key], g.recv, g.n, f"{name} {key}: isolated rows")
    for key in ("dh", "dpos"):
        bound = grad_row_bound(ref64[key], GRAD_BAR).expand_as(ref64[key])
        assert_within(got[key], ref64[key], bound, f"{name} {key}")
    for key in ("m_aggr", "pos_aggr", "dh", "dpos"):
        e[key] = (got[key].detach().cpu().double() - ref64[key]).abs().max().item()
    for k, want in ref64["grads"].items():  # tests/test_gpu_egnn.py::_assert_grads
        a = got["grads"][k].detach().cpu().double()
        scale = want.abs().max().item() + 1e-6
        err = (a - want).abs().max().item()
        print(f"{name} grad {k}: max|d| = {err:.3e}, scale {scale:.3e}")
        assert err <= 1e-4 * scale + 1e-6, f"{name} {k}: max|d|={err:.3e} scale={scale:.3e}"
        e[k] = err
    return e
