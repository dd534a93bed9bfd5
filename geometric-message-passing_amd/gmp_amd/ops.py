"""Thin, checked wrappers over the C ABI (include/gmp.h) + autograd Functions.

Every op launches on the current PyTorch HIP stream, allocates its outputs through the PyTorch
caching allocator and never synchronises.  Inputs must be CUDA (HIP) tensors: there is no CPU
fallback in the product path.
"""
import ctypes


import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-kernel timing (bench.py): name -> list of (start, end) HIP events recorded on the
# stream the kernel is launched on (the current stream).  None = disabled (no overhead).
KERNEL_TIMERS = None
KERNEL_TIMER_NAMES = None  # None: every timed region; else only these names (host cost: two
                           # event records per region, on the launch path)


class _timed:
    def __init__(self, name):
        self.name = name
        self.on = KERNEL_TIMERS is not None and (KERNEL_TIMER_NAMES is None
                                                 or name in KERNEL_TIMER_NAMES)

    def __enter__(self):
        if self.on:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.ev[1].record()
            KERNEL_TIMERS.setdefault(self.name, []).append(self.ev)
        return False


def kernel_time_ms(name):
    """Average device time (ms) per launch of a timed kernel, over the recorded launches."""
    evs = (KERNEL_TIMERS or {}).get(name, [])
    if not evs:
        return None
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) / len(evs)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.GmpError("gmp_amd ops run on the MI355X only: got a CPU tensor "
                                "(no CPU fallback in the product path)")


def _f32c(t):
    if t.dtype != torch.float32:
        raise _lib.GmpError(f"expected float32, got {t.dtype}")
    return t.contiguous()


def _i64c(t):
    if t.dtype != torch.int64:
        t = t.long()
    return t.contiguous()


# ----------------------------------------------------------------------------------- CSR
class CSR:
    """Stable CSR of an index array (gmp_csr_build): items sorted by index value.

    perm[k]   : original position of the k-th item in sorted order
    rowptr[s] : first sorted position with index >= s  (len n_seg + 1)
    sorted    : index[perm]; payload_sorted: payload[perm] (if a payload was given)
    """

    __slots__ = ("index", "n_seg", "perm", "rowptr", "sorted", "payload_sorted", "err")

    def __init__(self, index, n_seg, payload=None):
        index = _i64c(index)
        _need_cuda(index)
        self.index = index
        self.n_seg = int(n_seg)
        pl = _i64c(payload) if payload is not None else None
        self.perm, self.rowptr, self.sorted, pls, self.err = _lib.torch_ops().csr_build(
            index, self.n_seg, pl)
        self.payload_sorted = pls if pl is not None else None

    def counts(self):
        return self.rowptr[1:] - self.rowptr[:-1]

    def check_range(self):
        """Host-synchronising range check (torch_scatter raises on out-of-range indices)."""
        if int(self.err.item()) != 0:
            raise IndexError("index out of range in gmp CSR build")


_CSR_CACHE = []  # [(key, index_tensor, payload_tensor, CSR)] small LRU; holds strong refs


def _tkey(t):
    """Content identity of a (possibly view) tensor while a strong ref is held: storage
    address, geometry and the version counter shared with its base (in-place writes bump it).
    Views such as edge_index[1] taken repeatedly map to the same key."""
    if t is None:
        return None
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype, t.device, t._version)


def get_csr(index, n_seg, payload=None):
    """Cached CSR for `index` (keyed on storage/geometry/version; holds a strong ref)."""
    if compiling():
        return CSR(index, n_seg, payload)
    key = (_tkey(index), int(n_seg), _tkey(payload))
    for k, (kk, _, _, csr) in enumerate(_CSR_CACHE):
        if kk == key:
            _CSR_CACHE.insert(0, _CSR_CACHE.pop(k))
            return csr
    csr = CSR(index, n_seg, payload)
    _CSR_CACHE.insert(0, (key, index, payload, csr))
    del _CSR_CACHE[16:]
    return csr


def clear_cache():
    _CSR_CACHE.clear()


# ----------------------------------------------------------------------------------- raw ops
def gather_rows(src2d, index):
    src2d = _f32c(src2d)
    index = _i64c(index)
    _need_cuda(src2d, index)
    return _lib.torch_ops().gather_rows(src2d, index)


def segment_reduce(src2d, csr, reduce="sum", use_perm=True):
    """(out, argmax or None) = torch.ops.gmp.segment_reduce over the CSR's segments."""
    src2d = _f32c(src2d)
    _need_cuda(src2d)
    out, argmax = _lib.torch_ops().segment_reduce(src2d, csr.perm if use_perm else None,
                                                  csr.rowptr, csr.n_seg, reduce)
    return out, (argmax if reduce == "max" else None)


def edge_outer_sum(A, B):
    """(A^T B, colsum(A)) over the edge dimension (torch.ops.gmp.edge_outer_sum), deterministic."""
    A, B = _f32c(A), _f32c(B)
    _need_cuda(A, B)
    with _timed("edge_outer_sum"):
        return _lib.torch_ops().edge_outer_sum(A, B)


def edge_outer_sum_act(A, X, w, b, act, amax=None):
    """(A^T act(X * w + b), colsum(A)) with the activation applied at load time
    (torch.ops.gmp.edge_outer_sum_act): the EGNN y1 / m weight-gradient operands from x_hat.
    With `amax` (device word, max |A| as float bits; X LayerNorm rows) the HF form (scaled fp16
    planes, three products)."""
    A, X, w, b = _f32c(A), _f32c(X), _f32c(w), _f32c(b)
    _need_cuda(A, X, w, b)
    with _timed("edge_outer_sum"):
        return _lib.torch_ops().edge_outer_sum_act(A, X, w, b, _lib.ACT[act], amax)


def outer_sum_into(A, B, C, colsum=None, act=None, w=None, b=None):
    """C[:] = A^T act(B) over the rows (torch.ops.gmp.edge_outer_sum_ex), colsum[:] =
    colsum(A).  A (K, m), B (K, n) and C (m, n) may be strided views (unit column stride; e.g.
    column blocks of a wider tensor or parameter gradient).  Shapes outside the kernels' tile
    buckets run the library GEMM inside the op."""
    _need_cuda(A, B, C)
    a = -1 if act is None else _lib.ACT[act]
    with _timed("edge_outer_sum"):
        _lib.torch_ops().edge_outer_sum_ex(A, B, C, colsum, a, w, b)


def outer_sum_into2(A, B1, B2, C, colsum=None):
    """C[:] = A^T [B1 | B2] (and colsum(A)) in one pass over A where the split-plane kernel
    applies, else as two products inside the op."""
    _need_cuda(A, B1, B2, C)
    with _timed("edge_outer_sum"):
        _lib.torch_ops().edge_outer_sum_ex2(A, B1, B2, C, colsum)


def edge_outer_sum_rect(A, B):
    """(A^T B, colsum(A)) over the rows (edges / nodes) for any widths, deterministic: columns
    zero-padded to multiples of 16 when needed, wide operands processed as <= 128 x 144 column
    blocks read in place (strided) and written into their block of C."""
    A, B = _f32c(A), _f32c(B)
    _need_cuda(A, B)
    m, n = A.shape[1], B.shape[1]
    mp, np_ = -(-m // 16) * 16, -(-n // 16) * 16
    if mp != m:
        A = torch.nn.functional.pad(A, (0, mp - m))
    if np_ != n:
        B = torch.nn.functional.pad(B, (0, np_ - n))
    C = torch.empty((mp, np_), dtype=torch.float32, device=A.device)
    cs = torch.empty(mp, dtype=torch.float32, device=A.device)
    bn = 144 if np_ <= 144 else 128
    for m0 in range(0, mp, 128):
        for n0 in range(0, np_, bn):
            outer_sum_into(A[:, m0:m0 + 128], B[:, n0:n0 + bn], C[m0:m0 + 128, n0:n0 + bn],
                           cs[m0:m0 + 128] if n0 == 0 else None)
    if (mp, np_) != (m, n):
        return C[:m, :n].contiguous(), cs[:m]
    return C, cs


# ----------------------------------------------------------------------------------- deferred
# Weight gradients are leaves of the backward graph: nothing downstream waits for them.  They
# are computed on a side stream (overlapping the critical path's small node-level kernels and
# the host launch gaps between them) and accumulated into param.grad by a callback at the end
# of the backward pass, as DDP does with its reducer.  Disable (DEFER_WEIGHT_GRADS = False)
# when something must see these gradients through autograd (DDP's per-parameter hooks);
# gmp_amd.dist.wrap_ddp does so.  Under torch.autograd.grad (the engine runs no AccumulateGrad)
# they are returned through autograd automatically (_engine_accumulates).
DEFER_WEIGHT_GRADS = True
_SIDE_STREAMS = {}
_PENDING = []   # (param, grad) accumulated at the end of the backward pass
_CB_QUEUED = [False]
# Main-stream tensors read by side-stream work are kept alive here until the main stream has
# waited for the side stream (flush / join), then dropped: their blocks go straight back to the
# main stream's pool, stream-ordered after that wait.  (record_stream instead would hold every
# such block until the allocator sees the side stream's event complete; with the host running a
# step ahead it then allocated fresh HBM every step and synchronised the host doing so.)
_KEEPALIVE = []


def _side_stream(device):
    st = _SIDE_STREAMS.get(device)
    if st is None:
        st = _SIDE_STREAMS[device] = torch.cuda.Stream(device=device)
    return st


def _flush_deferred():
    _CB_QUEUED[0] = False
    if not _PENDING:
        return
    main = torch.cuda.current_stream()
    for st in _SIDE_STREAMS.values():
        main.wait_stream(st)
    _KEEPALIVE.clear()
    for p, g in _PENDING:
        g.record_stream(main)
        if p.grad is None:
            # AccumulateGrad's layout contract: a dense gradient with the parameter's strides
            p.grad = g if g.stride() == p.stride() else g.contiguous()
        else:
            p.grad.add_(g)
    _PENDING.clear()


def deferrable(t):
    return DEFER_WEIGHT_GRADS and t is not None and t.is_leaf and t.requires_grad


def _engine_accumulates(p):
    """True when the running backward pass will execute p's AccumulateGrad (loss.backward());
    False under torch.autograd.grad, which either skips the parameter or captures its gradient
    as an output — then the gradient must travel through autograd, not into p.grad."""
    try:
        with torch.enable_grad():
            acc = p.view_as(p).grad_fn.next_functions[0][0]
        return bool(torch._C._will_engine_execute_node(acc))
    except (RuntimeError, AttributeError, IndexError):
        return False


def compiling():
    """True while torch.compile (dynamo) traces: the ops then run inline on the current stream,
    without the per-graph caches, side streams or end-of-backward callbacks of eager mode."""
    return torch.compiler.is_compiling()


class side_work:
    """with side_work(used_tensors) as sw: ... launches on the side stream after everything
    already queued on the current stream; sw.deliver(...) hands each result to the end-of-
    backward accumulation (deferred leaf gradients) or back through autograd (after joining the
    streams).  Under torch.compile the work runs inline and every gradient goes back through
    autograd."""

    def __init__(self, *used):
        self.used = [t for t in used if t is not None]
        self.inline = compiling()

    def __enter__(self):
        if self.inline:
            return self
        self.main = torch.cuda.current_stream()
        self.side = _side_stream(self.main.device)
        self.side.wait_stream(self.main)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.inline:
            return False
        self.ctx.__exit__(*exc)
        _KEEPALIVE.extend(self.used)
        return False

    def defer(self, param, grad):
        _PENDING.append((param, grad))
        if not _CB_QUEUED[0]:
            _CB_QUEUED[0] = True
            torch.autograd.Variable._execution_engine.queue_callback(_flush_deferred)

    def join(self, *results):
        """results are needed on the current stream now (returned through autograd)."""
        self.main.wait_stream(self.side)
        _KEEPALIVE.clear()
        for r in results:
            if r is not None:
                r.record_stream(self.main)

    def deliver(self, needs_input_grad, first, targets, grads):
        """Per parameter: defer the gradient (leaf parameter) or hand it back through autograd
        (after joining the streams).  needs_input_grad[first + i] belongs to targets[i]."""
        if self.inline:
            return tuple(gr if needs_input_grad[first + i] else None
                         for i, gr in enumerate(grads))
        out, joined, deferred = [], False, False
        accum = None  # does this backward pass accumulate into .grad (checked once per call)
        for i, (p, gr) in enumerate(zip(targets, grads)):
            if deferrable(p) and needs_input_grad[first + i] and accum is None:
                accum = _engine_accumulates(p)
            if not needs_input_grad[first + i]:
                out.append(None)
            elif deferrable(p) and accum:
                self.defer(p, gr)
                deferred = True
                out.append(None)
            else:
                if not joined:
                    self.join(*[g for g in grads if g is not None])
                    joined = True
                out.append(gr)
        if not (joined or deferred):
            # no parameter gradient wanted (e.g. autograd.grad w.r.t. inputs only): nothing will
            # flush this side work, so join here and release the kept-alive inputs
            self.main.wait_stream(self.side)
            _KEEPALIVE.clear()
        return tuple(out)


def _mm_wt(g, Wt):
    """g @ Wt.t() for a contiguous Wt (n, k): the library GEMM's "NT" form, measured ~1.5x
    faster than the "NN" g @ W for the (50k x 128) x (128 x 128) node GEMMs (22.5 vs 34 us);
    the transposed weight copy is one small kernel."""
    return g.mm(Wt.t())


def _dx(g, W):
    """g @ W for the dx of y = x W^T (W (n_out, n_in))."""
    return _mm_wt(g, W.t().contiguous())


class EdgeLinearFn(torch.autograd.Function):
    """y = x W^T (+ b) over many rows (edges): forward and dx with the library GEMM (M = rows),
    dW / db with the deterministic edge outer sum (K = rows), which the library's small-tile
    K-reduction GEMMs run far below the HBM roofline.  dW / db of leaf parameters are computed
    on the side stream and accumulated at the end of the backward pass (deferred)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W, b)
        return torch.addmm(b, x, W.t()) if b is not None else x.mm(W.t())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W, b = ctx.saved_tensors
        g = g.contiguous()
        dx = _dx(g, W) if ctx.needs_input_grad[0] else None
        need_w = ctx.needs_input_grad[1] or (b is not None and ctx.needs_input_grad[2])
        if not need_w:
            return dx, None, None
        with side_work(g, x) as sw:
            dW, db = edge_outer_sum_rect(g, x)
        return (dx,) + sw.deliver(ctx.needs_input_grad, 1, (W, b), (dW, db))


class SplitLinearFn(torch.autograd.Function):
    """y = [xa | xb] W^T + b without materialising the concatenation (egnn_layer.py:37
    mlp_upd[0] over cat([h, m_aggr])): two GEMMs forward, two for dx; dW written block-wise
    into one (out, ina + inb) gradient by the strided outer sum (deferred for leaf params)."""

    @staticmethod
    def forward(ctx, xa, xb, W, b):
        da = xa.shape[1]
        ctx.save_for_backward(xa, xb, W, b)
        y = torch.addmm(b, xa, W[:, :da].t()) if b is not None else xa.mm(W[:, :da].t())
        y.addmm_(xb, W[:, da:].t())
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xa, xb, W, b = ctx.saved_tensors
        da = xa.shape[1]
        g = g.contiguous()
        dxa = _dx(g, W[:, :da]) if ctx.needs_input_grad[0] else None
        dxb = _dx(g, W[:, da:]) if ctx.needs_input_grad[1] else None
        need_w = ctx.needs_input_grad[2] or (b is not None and ctx.needs_input_grad[3])
        if not need_w:
            return dxa, dxb, None, None
        with side_work(g, xa, xb) as sw:
            dW = torch.empty_like(W)
            db = torch.empty(W.shape[0], dtype=W.dtype, device=W.device)
            outer_sum_into(g, xa, dW[:, :da], db)
            outer_sum_into(g, xb, dW[:, da:], None)
        return (dxa, dxb) + sw.deliver(ctx.needs_input_grad, 2, (W, b), (dW, db))


def split_linear(xa, xb, W, b=None):
    """F.linear(cat([xa, xb], -1), W, b) for 2-D inputs without the concatenation."""
    if (xa.is_cuda and xa.dim() == 2 and xb.dim() == 2 and xa.dtype == torch.float32
            and xa.shape[0] >= EDGE_LINEAR_MIN_ROWS and xa.shape[1] % 4 == 0
            and xb.shape[1] % 4 == 0):
        return SplitLinearFn.apply(xa.contiguous(), xb.contiguous(), W, b)
    return torch.nn.functional.linear(torch.cat([xa, xb], -1), W, b)


_LN_ACT = {"relu": 0, "swish": 1, "silu": 1, None: 2, "identity": 2}


class LnActFn(torch.autograd.Function):
    """act(LayerNorm(x)) over the last dim (K12 gmp_ln_act_*): one fused kernel each way,
    deterministic gamma/beta gradients."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act):
        shape = x.shape
        d = shape[-1]
        x2 = _f32c(x).reshape(-1, d)
        gamma, beta = _f32c(gamma), _f32c(beta)
        _need_cuda(x2, gamma, beta)
        a = _LN_ACT[act]
        y, xhat, rstd = _lib.torch_ops().ln_act_fwd(x2, gamma, beta, float(eps), a)
        ctx.save_for_backward(xhat, rstd, gamma, beta)
        ctx.act, ctx.shape = a, shape
        return y.view(shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        xhat, rstd, gamma, beta = ctx.saved_tensors
        rows, d = xhat.shape
        gy = _f32c(gy).reshape(rows, d)
        # (deferring the [dgamma | dbeta] reduction to the side stream was measured slower: the
        # extra stream bookkeeping lengthens the host-bound stretch of small node kernels)
        gx, gb = _lib.torch_ops().ln_act_bwd(gy, xhat, rstd, gamma, beta, ctx.act)
        return gx.view(ctx.shape), gb[:d], gb[d:], None, None


def ln_act(x, ln, act=None):
    """act(ln(x)) for an nn.LayerNorm `ln` (affine) through K12."""
    return LnActFn.apply(x, ln.weight, ln.bias, ln.eps, act)


EDGE_LINEAR_MIN_ROWS = 1 << 15


def linear(x, W, b=None):
    """F.linear for (..., in) inputs; row counts >= EDGE_LINEAR_MIN_ROWS on the GPU take the
    EdgeLinearFn path (deterministic outer-sum weight gradients)."""
    shp = x.shape
    x2 = x.reshape(-1, shp[-1])
    if x2.is_cuda and x2.shape[0] >= EDGE_LINEAR_MIN_ROWS and x2.dtype == torch.float32:
        fn = EdgeLinear2Fn if _SECOND_ORDER[0] else EdgeLinearFn
        y = fn.apply(x2.contiguous(), W, b)
    else:
        y = torch.nn.functional.linear(x2, W, b)
    return y.reshape(shp[:-1] + (W.shape[0],))


def segment_reduce_bwd(grad_out, csr, reduce, argmax, n_items):
    return _lib.torch_ops().segment_reduce_bwd(_f32c(grad_out), csr.index, csr.rowptr, reduce,
                                               argmax, n_items)


# ----------------------------------------------------------------------------------- autograd
class SegmentReduceFn(torch.autograd.Function):
    """out[s] = reduce_{e: index[e]==s} src[e]   (torch_scatter.scatter along dim 0)."""

    @staticmethod
    def forward(ctx, src2d, csr, reduce):
        out, argmax = segment_reduce(src2d, csr, reduce)
        ctx.csr, ctx.reduce, ctx.n = csr, reduce, src2d.shape[0]
        ctx.save_for_backward(argmax if argmax is not None else torch.empty(0))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (argmax,) = ctx.saved_tensors
        gs = segment_reduce_bwd(g.contiguous(), ctx.csr, ctx.reduce,
                                argmax if ctx.reduce == "max" else None, ctx.n)
        return gs, None, None


class SegmentMaxFn(torch.autograd.Function):
    """(out, argmax) of a segmented max (torch_scatter.scatter_max along dim 0): the gradient
    goes to the arg-max item of each (segment, feature); argmax is not differentiable."""

    @staticmethod
    def forward(ctx, src2d, csr):
        out, argmax = segment_reduce(src2d, csr, "max")
        ctx.csr, ctx.n = csr, src2d.shape[0]
        ctx.save_for_backward(argmax)
        ctx.mark_non_differentiable(argmax)
        return out, argmax

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_arg):
        (argmax,) = ctx.saved_tensors
        return segment_reduce_bwd(g.contiguous(), ctx.csr, "max", argmax, ctx.n), None


class GatherRowsFn(torch.autograd.Function):
    """out[e] = src[index[e]]; backward = deterministic segmented sum over the CSR of index."""

    @staticmethod
    def forward(ctx, src2d, index, n_rows):
        ctx.index, ctx.n_rows = index, n_rows
        return gather_rows(src2d, index)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        csr = get_csr(ctx.index, ctx.n_rows)
        out, _ = segment_reduce(g.contiguous(), csr, "sum")
        return out, None, None


def gather(src, index, dim=0):
    """index_select(src, dim, index) through the HIP gather kernel (differentiable)."""
    dim = dim % src.dim()
    x = src.movedim(dim, 0)
    shp = x.shape
    x2 = x.reshape(shp[0], -1)
    out = (GatherRows2Fn if _SECOND_ORDER[0] else GatherRowsFn).apply(x2, index, shp[0])
    return out.reshape((index.numel(),) + tuple(shp[1:])).movedim(0, dim)


# ----------------------------------------------------------------------------------- CFConv
_CHECKED_CSR = []  # CSRs whose build-time range flag was already read (once per graph)


def checked_csr(index, n):
    """get_csr plus the build's out-of-range flag read once per new graph (one host sync, as
    torch_scatter raises for an index outside the output rows fixed by dim_size / out=)."""
    csr = get_csr(index, n)
    if compiling():
        return csr
    if not any(c is csr for c in _CHECKED_CSR):
        csr.check_range()  # one host sync per new graph, as torch_scatter raises IndexError
        _CHECKED_CSR.insert(0, csr)
        del _CHECKED_CSR[32:]
    return csr


_cfconv_csr = checked_csr


def cfconv_aggregate(x, xidx, w, csr, escale=None):
    """out[s] = sum over CSR segment s of x[xidx[e]] * (w[e] (* escale[e])) (K13
    gmp_cfconv_aggregate_scaled_f32)."""
    return _lib.torch_ops().cfconv_aggregate(x, _i64c(xidx), w, csr.perm, csr.rowptr, csr.n_seg,
                                             escale)


class CFConvAggregateFn(torch.autograd.Function):
    """PyG CFConv propagate (message x_j * W, aggr "add", dim_size = N; schnet.py:72) without
    the (E, F) message: forward and x-gradient by K13 over the receiver / sender CSR, the
    W-gradient as the per-edge product grad[dst] * x[src].  C (optional, no gradient): the
    per-edge cosine cutoff multiplying W (W * C.view(-1, 1) in CFConv.forward), applied at load
    time; the W-gradient is then the gradient w.r.t. the unscaled W."""

    @staticmethod
    def forward(ctx, x, W, src, dst, n, C=None):
        recv = _cfconv_csr(dst, n)
        ctx.save_for_backward(x, W, C)
        ctx.src, ctx.dst, ctx.n = src, dst, n
        return cfconv_aggregate(x, src, W, recv, C)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W, C = ctx.saved_tensors
        g = _f32c(g)
        dx = dW = None
        if ctx.needs_input_grad[0]:
            dx = cfconv_aggregate(g, ctx.dst, W, _cfconv_csr(ctx.src, x.shape[0]), C)
        if ctx.needs_input_grad[1]:
            dW = _lib.torch_ops().cfconv_wgrad(g, _i64c(ctx.dst), x, _i64c(ctx.src), C)
        if ctx.needs_input_grad[5]:
            raise RuntimeError("cfconv_propagate: C must not require grad (use W * C instead)")
        return dx, dW, None, None, None, None


class ShiftedSoftplusFn(torch.autograd.Function):
    """softplus(x) - shift in one pass each way (K14 gmp_ssp_{fwd,bwd}_f32)."""

    @staticmethod
    def forward(ctx, x, shift):
        y = _lib.torch_ops().ssp_fwd(x, float(shift))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _f32c(g)
        if g.data_ptr() % 16:  # a contiguous view at an odd offset: K14 needs 16-byte rows
            g = g.clone()
        return _lib.torch_ops().ssp_bwd(x, g), None


def shifted_softplus(x, shift):
    """F.softplus(x) - shift through K14 (CUDA fp32, numel % 4 == 0, 16-byte aligned)."""
    x = _f32c(x)
    _need_cuda(x)
    return (ShiftedSoftplus2Fn if _SECOND_ORDER[0] else ShiftedSoftplusFn).apply(x, shift)


def cfconv_propagate(edge_index, x, W, C=None):
    """sum_{e: dst[e] = i} x[src[e]] * W[e] (* C[e]) for edge_index = (src, dst), N =
    x.shape[0]; C (E,) is a per-edge factor without gradient (SchNet's cosine cutoff).  Inside
    second_order() the twice-differentiable form is recorded and C may require grad."""
    x, W = _f32c(x), _f32c(W)
    _need_cuda(x, W)
    if _SECOND_ORDER[0]:
        ei = _i64c(edge_index)
        return cfconv_receiver_aggregate(x, W, None if C is None else C.reshape(-1), ei[0],
                                         ei[1], x.shape[0])
    if C is not None:
        if C.requires_grad and torch.is_grad_enabled():
            raise ValueError("cfconv_propagate: C must not require grad")
        C = _f32c(C.detach().reshape(-1))
    ei = _i64c(edge_index)
    return CFConvAggregateFn.apply(x, W, ei[0], ei[1], x.shape[0], C)


# ----------------------------------------------------------------------------------- K1 edges
def edge_vec_to_pos_grad(g_vec, edge_index, n):
    """d pos from d vec for vec = pos[ei0] - pos[ei1]: deterministic segmented sums over the
    cached CSRs of ei0 (+) and ei1 (-)."""
    plus, _ = segment_reduce(g_vec, get_csr(edge_index[0], n), "sum")
    minus, _ = segment_reduce(g_vec, get_csr(edge_index[1], n), "sum")
    return plus - minus


class GvpEdgeFeaturizeFn(torch.autograd.Function):
    """GVP-GNN edge features (gvpgnn.py:106-112) in one pass over the edges (K1,
    gmp_edge_featurize_gvp_f32): (radial (E, nb), unit vectors nan_to_num(vec / |vec|) (E, 3))."""

    @staticmethod
    def forward(ctx, pos, edge_index, host_consts):
        w, pref, r_max, p = host_consts
        pos, ei = _f32c(pos), _i64c(edge_index)
        _need_cuda(pos, ei)
        with _timed("edge_featurize"):
            rad, unit = _lib.torch_ops().edge_featurize_gvp(pos, ei, [float(v) for v in w], pref,
                                                            r_max, p)
        ctx.save_for_backward(pos, ei)
        ctx.host = host_consts
        return rad, unit

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rad, g_unit):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        pos, ei = ctx.saved_tensors
        w, pref, r_max, p = ctx.host
        g_vec = _lib.torch_ops().edge_featurize_gvp_bwd(
            pos, ei, [float(v) for v in w], pref, r_max, p,
            _f32c(g_rad) if g_rad is not None else None,
            _f32c(g_unit) if g_unit is not None else None)
        return edge_vec_to_pos_grad(g_vec, ei, pos.shape[0]), None, None


def _needs(ctx, k):
    """needs_input_grad[k] of an optional trailing input (absent: False)."""
    return len(ctx.needs_input_grad) > k and ctx.needs_input_grad[k]


class SchNetFeaturizeFn(torch.autograd.Function):
    """SchNet edge features (schnet.py:66-68 over PyG SchNet.forward / GaussianSmearing /
    CFConv.forward) in one pass over the edges (gmp_schnet_featurize_f32): edge_weight (E),
    Gaussians (E, G) and the CFConv cosine cutoff C (E).  shift (E, 3), if given, is added to the
    edge vector (periodic images); its cotangent is g_vec."""

    @staticmethod
    def forward(ctx, pos, edge_index, offsets, coeff, cutoff, shift=None):
        pos, ei, off = _f32c(pos), _i64c(edge_index), _f32c(offsets)
        _need_cuda(pos, ei, off)
        sh = _f32c(shift) if shift is not None else None
        with _timed("edge_featurize"):
            d, rbf, cut = _lib.torch_ops().schnet_featurize(pos, ei, off, float(coeff),
                                                            float(cutoff), sh)
        ctx.save_for_backward(pos, ei, off, sh)
        ctx.coeff, ctx.cutoff = float(coeff), float(cutoff)
        return d, rbf, cut

    @staticmethod
    @once_differentiable
    def backward(ctx, g_d, g_rbf, g_cut):
        need_pos, need_shift = ctx.needs_input_grad[0], _needs(ctx, 5)
        if not (need_pos or need_shift):
            return None, None, None, None, None, None
        pos, ei, off, sh = ctx.saved_tensors
        opt = [_f32c(t) if t is not None else None for t in (g_d, g_rbf, g_cut)]
        g_vec = _lib.torch_ops().schnet_featurize_bwd(pos, ei, off, ctx.coeff, ctx.cutoff, *opt,
                                                      sh)
        return (edge_vec_to_pos_grad(g_vec, ei, pos.shape[0]) if need_pos else None, None, None,
                None, None, g_vec if need_shift else None)


# ----------------------------------------------------------------------------------- EGNN
class EgnnGraph:
    """Receiver-sorted view of an edge_index for the fused EGNN kernels (built on device)."""

    def __init__(self, edge_index, num_nodes):
        ei = _i64c(edge_index)
        _need_cuda(ei)
        self.num_nodes = int(num_nodes)
        self.num_edges = ei.shape[1]
        self.recv_csr = CSR(ei[1], self.num_nodes, payload=ei[0])
        self.recv = self.recv_csr.sorted             # receiver of sorted edge k
        self.send = self.recv_csr.payload_sorted     # sender of sorted edge k
        self.rowptr = self.recv_csr.rowptr
        self.send_csr = CSR(self.send, self.num_nodes)  # sender CSR over sorted positions

    def check_range(self):
        """Host-synchronising check that every edge_index entry is in [0, num_nodes)."""
        self.recv_csr.check_range()
        self.send_csr.check_range()


_EGNN_GRAPHS = []


def egnn_graph(edge_index, num_nodes):
    if compiling():
        return EgnnGraph(edge_index, num_nodes)
    for k, (t, ver, n, g) in enumerate(_EGNN_GRAPHS):
        if t is edge_index and ver == edge_index._version and n == num_nodes:
            return g
    g = EgnnGraph(edge_index, num_nodes)
    _EGNN_GRAPHS.insert(0, (edge_index, edge_index._version, num_nodes, g))
    del _EGNN_GRAPHS[8:]
    return g


_EGNN_PARAM_NAMES = ("w1d", "b1", "ln1_w", "ln1_b", "W2", "b2", "ln2_w", "ln2_b", "W3", "b3",
                     "ln3_w", "ln3_b", "w4", "b4")


def _egnn_params(tensors):
    return _lib.GmpEgnnParams(*[t.data_ptr() for t in tensors])


# LayerNorm outputs the EGNN forward saves for the backward: 2 = x_hat1, x_hat2 (x_hat3 recomputed
# in the backward, bitwise the forward's), 3 = x_hat1..3 (the r02 form; tests compare the two).
# The backward follows the saved tensor's plane count.
EGNN_XHAT_PLANES = 2

# True: EgnnMessageFn leaves out the work nobody reads — the mlp_pos branch of a layer whose
# position output is unused (need_pos=False in the forward; in the backward whenever no gradient
# arrives for pos_aggr: kernels without the W3 products, no dW3 / db3 outer sum) and the position
# gradient when pos does not require grad (no gdiff, no sender-side reduction).  Results are
# bitwise those of False, which runs the full kernels everywhere (the A/B and the tests).
EGNN_SKIP_DEAD_POS = True


class EgnnMessageFn(torch.autograd.Function):
    """The whole EGNN message block of one layer (egnn_layer.py:62-80 with the MLPs of :28-36):
    the node projections AB = [h W1a^T | h W1b^T] (one GEMM), the fused edge kernel K4 and the
    aggregation; backward = K4 backward, sender-side segmented sums, dh on the critical path,
    and every weight gradient (dW1 assembled in place as [dW1a | dW1b | dw1d], dW2, dW3 via
    the edge outer sums, LayerNorm / vector partials) on the side stream, deferred.

    Parameters in module order: mlp_msg.0.{weight (d, 2d+1), bias}, mlp_msg.1.{weight, bias},
    mlp_msg.3.{weight, bias}, mlp_msg.4.{weight, bias}, mlp_pos.0.{weight, bias},
    mlp_pos.1.{weight, bias}, mlp_pos.3.{weight (1, d), bias}.
    Returns (m_aggr (N, d), pos_aggr (N, 3)); need_pos=False (the caller drops this layer's
    position output, e.g. the model's last layer without equivariant_pred): (m_aggr, None), and
    mlp_pos receives zero gradients.  AB: the node projections precomputed by the
    previous layer's K15 node update (EgnnNodeFn), a constant here: the gradient w.r.t. h still
    comes from this Function's backward (dh = [dA | dB] [W1a ; W1b]).
    """

    @staticmethod
    def forward(ctx, h, pos, graph, act, msg_mean, eps, W1, b1, ln1w, ln1b, W2, b2, ln2w, ln2b,
                W3, b3, ln3w, ln3b, w4, b4, grad_mode=True, AB=None, need_pos=True):
        h, pos = _f32c(h), _f32c(pos)
        _need_cuda(h, pos, W1)
        N, d = h.shape
        E = graph.num_edges
        if AB is None:  # [h W1a^T | h W1b^T] (else: K15 produced it with the previous update)
            Wcat = torch.cat([W1[:, :d], W1[:, d:2 * d]], 0)
            AB = h.mm(Wcat.t())
        params = tuple(_f32c(t) for t in (W1[:, 2 * d], b1, ln1w, ln1b, W2, b2, ln2w, ln2b, W3,
                                          b3, ln3w, ln3b, w4, b4))
        # save the LayerNorm outputs only for a backward: grad_mode is the CALLER's
        # torch.is_grad_enabled() (forward() itself always runs with grad disabled, and
        # needs_input_grad follows requires_grad alone: r04's inference forward saved 1 GB of
        # x_hat planes per layer under torch.no_grad)
        train = bool(grad_mode) and any(ctx.needs_input_grad)
        # a None g_p in backward then means that nobody used the position output
        ctx.set_materialize_grads(False)
        fwd_pos = bool(need_pos) or not EGNN_SKIP_DEAD_POS
        with _timed("egnn_edge_fwd"):
            m_aggr, pos_aggr, xhat, rstd = _lib.torch_ops().egnn_edge_fwd(
                AB, pos, graph.rowptr, graph.recv, graph.send, list(params), _lib.ACT[act],
                bool(msg_mean), float(eps), train, EGNN_XHAT_PLANES, fwd_pos)
        ctx.graph, ctx.act, ctx.msg_mean, ctx.N = graph, act, msg_mean, N
        ctx.fwd_pos = fwd_pos  # False: rstd[:, 2] (and x_hat3) were not written
        if train:
            ctx.save_for_backward(h, pos, xhat, rstd, W1, *params)
        return m_aggr, (pos_aggr if need_pos else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_m, g_p):
        h, pos, xhat, rstd, W1, *params = ctx.saved_tensors
        graph = ctx.graph
        N, d = ctx.N, xhat.shape[2]
        E = graph.num_edges
        dev = pos.device
        f = dict(dtype=torch.float32, device=dev)
        # static per call site (no data-dependent branch): the position branch only where it ran
        # in the forward and a gradient arrives for it; the position gradient only where asked for
        pos_branch = ctx.fwd_pos and not (EGNN_SKIP_DEAD_POS and g_p is None)
        pos_grad = ctx.needs_input_grad[1] or not EGNN_SKIP_DEAD_POS
        g_m = torch.zeros((N, d), **f) if g_m is None else _f32c(g_m)
        if not pos_branch:
            g_p = torch.empty((0, 3), **f)  # (not read)
        else:
            g_p = torch.zeros((N, 3), **f) if g_p is None else _f32c(g_p)
        # HF weight-gradient outer sums: the backward kernel folds max |dpre2|, |dpre3| into
        # two device words that scale their fp16 planes
        amax = torch.zeros(2, dtype=torch.int32, device=dev)
        with _timed("egnn_edge_bwd"):
            dA, dpos_recv, dpre1, gdiff, dpre2, dpre3, partials = \
                _lib.torch_ops().egnn_edge_bwd(pos, graph.rowptr, graph.recv, graph.send,
                                               list(params), _lib.ACT[ctx.act],
                                               bool(ctx.msg_mean), xhat, rstd, g_m, g_p, amax,
                                               pos_branch, pos_grad)
        xh1, xh2 = xhat[0], xhat[1]  # for the dW2 / dW3 sums
        # critical path: sender-side sums (deterministic, sender CSR) and dh
        dB, _ = segment_reduce(dpre1, graph.send_csr, "sum")
        W1t = W1[:, :2 * d].t().contiguous()  # [W1a | W1b]^T: NT-form GEMMs for dh
        dh = _mm_wt(dA, W1t[:d])
        dh.addmm_(dB, W1t[d:].t())
        dpos = None
        if pos_grad:
            dpos_send, _ = segment_reduce(gdiff, graph.send_csr, "sum")
            dpos = dpos_recv - dpos_send

        # weight gradients: side stream, accumulated at the end of the backward pass
        (_, b1, ln1w, ln1b, W2, b2, ln2w, ln2b, W3, b3, ln3w, ln3b, w4, b4) = params
        # the edge-level sums (dW2, dW3: ~0.2 ms each) inline on the main stream (r05): on the
        # side stream they took the CUs from the critical path's node-level backward kernels
        # (LayerNorm backward + its column sums 0.33 ms instead of ~0.04 ms per layer, trace);
        # A/B on one box, 20-step runs: 114.4 (113.7-115.0) vs 113.2 (112.9-113.4) M edges/s
        dW2, db2 = edge_outer_sum_act(dpre2, xh1, ln1w, ln1b, ctx.act, amax[0:1])
        if pos_branch:
            dW3, db3 = edge_outer_sum_act(dpre3, xh2, ln2w, ln2b, ctx.act, amax[1:2])
        else:  # the loss reaches none of mlp_pos: zeros, what the sum of a zero dpre3 gave
            dW3, db3 = torch.zeros((d, d), **f), torch.zeros(d, **f)
        with side_work(h, dA, dB, partials) as sw:
            dW1 = torch.empty((d, 2 * d + 1), **f)
            db1 = torch.empty(d, **f)
            outer_sum_into(dA, h, dW1[:, :d], db1)
            outer_sum_into(dB, h, dW1[:, d:2 * d])
            v = partials.sum(0)
            dln1w, dln1b, dln2w, dln2b, dln3w, dln3b, dw4, dw1d = v[:8 * d].view(8, d).unbind(0)
            dW1[:, 2 * d].copy_(dw1d)
            grads = (dW1, db1, dln1w, dln1b, dW2, db2, dln2w, dln2b, dW3, db3, dln3w, dln3b,
                     dw4.view(1, d), v[8 * d:8 * d + 1])
        # the caller's parameter tensors (saved tensors unpack to the same objects): W1 itself,
        # then b1 ... b4 (params[0] is the contiguous copy of W1's distance column)
        targets = (W1,) + tuple(params[1:])
        return (dh, dpos, None, None, None, None) + sw.deliver(ctx.needs_input_grad, 6, targets,
                                                               grads) + (None, None, None)


def egnn_exact_mode():
    """True while the EGNN kernels run their exact-f32 A/B mode (gmp_egnn_set_f32_mfma(1))."""
    lib = _lib.load()
    prev = lib.gmp_egnn_set_f32_mfma(0)
    lib.gmp_egnn_set_f32_mfma(prev)
    return bool(prev)


def egnn_node_images(layers, next_layers):
    """uint8 (L, bytes) K15 weight images (gmp_egnn_node_image_f32, one launch): per EGNN layer
    its mlp_upd.0 / mlp_upd.3 weights and the next layer's mlp_msg.0 weight (None: last layer).
    A constant for autograd (built from the current weights; rebuilt every forward)."""
    with torch.no_grad():
        return _lib.torch_ops().egnn_node_image(
            [_f32c(l.mlp_upd[0].weight) for l in layers], [_f32c(l.mlp_upd[3].weight) for l in layers],
            [None if n is None else n.mlp_msg[0].weight for n in next_layers])


# False: the node update's backward as the composed kernels (K12 LayerNorm backwards + library
# GEMMs; tests compare the two)
EGNN_NODE_BWD_FUSED = True


class EgnnNodeFn(torch.autograd.Function):
    """K15 (gmp_egnn_node_fwd_f32): the EGNN node update of one layer (egnn_layer.py:82-86,
    mlp_upd over [h | m_aggr]), the model's residual (egnn.py:75-76) and the next layer's node
    projections AB' = [h' W1a'^T | h' W1b'^T] in one launch, from the layer's weight image
    (egnn_node_images).  Returns (h', AB' or None) — AB' is a constant for autograd (the next
    EgnnMessageFn differentiates through h').  Backward: the LayerNorm + act backwards (K12) from
    the saved x_hat / 1/std, the dx GEMMs on the critical path, the weight gradients by the
    deterministic outer sums on the side stream (deferred), as the unfused SplitLinearFn /
    LnActFn / EdgeLinearFn chain does."""

    @staticmethod
    def forward(ctx, h, m, W0, b0, ln1w, ln1b, W3, b3, ln2w, ln2b, image, with_ab, act, residual,
                eps, grad_mode):
        h, m = _f32c(h), _f32c(m)
        _need_cuda(h, m, W0)
        vecs = [_f32c(t) for t in (b0, ln1w, ln1b, b3, ln2w, ln2b)]
        train = bool(grad_mode) and any(ctx.needs_input_grad)
        with _timed("egnn_node_fwd"):
            ho, ab, xhat, rstd = _lib.torch_ops().egnn_node_fwd(
                h, m, vecs, image, bool(with_ab), _lib.ACT[act], bool(residual), float(eps), train)
        ctx.act, ctx.residual = act, bool(residual)
        if train:
            ctx.save_for_backward(h, m, xhat, rstd, _f32c(W0), vecs[0], vecs[1], vecs[2],
                                  _f32c(W3), vecs[3], vecs[4], vecs[5])
        ctx.mark_non_differentiable(ab)
        return ho, (ab if with_ab else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_ab):
        h, m, xhat, rstd, W0, b0, ln1w, ln1b, W3, b3, ln2w, ln2b = ctx.saved_tensors
        d = h.shape[1]
        g = _f32c(g)
        tops = _lib.torch_ops()
        a = _LN_ACT[ctx.act]
        if EGNN_NODE_BWD_FUSED and a in (0, 1) and d in (32, 64, 128):
            # K15b: both LayerNorm + act backwards, the three dx products and the residual in
            # one launch (gmp_egnn_node_bwd_f32)
            with _timed("egnn_node_bwd"):
                dh, dm, dpre1, dpre2, gb = tops.egnn_node_bwd(g, xhat, rstd, W0, W3,
                                                              [ln1w, ln1b, ln2w, ln2b], a,
                                                              ctx.residual)
            gb1, gb2 = gb[:2 * d], gb[2 * d:]
            dh = dh if ctx.needs_input_grad[0] else None
            dm = dm if ctx.needs_input_grad[1] else None
        else:
            dpre2, gb2 = tops.ln_act_bwd(g, xhat[1], rstd[1], ln2w, ln2b, a)
            dx1 = _dx(dpre2, W3)
            dpre1, gb1 = tops.ln_act_bwd(dx1, xhat[0], rstd[0], ln1w, ln1b, a)
            dh = _dx(dpre1, W0[:, :d]) if ctx.needs_input_grad[0] else None
            if dh is not None and ctx.residual:
                dh += g
            dm = _dx(dpre1, W0[:, d:]) if ctx.needs_input_grad[1] else None
        with side_work(dpre1, dpre2, h, m, xhat) as sw:
            dW0 = torch.empty_like(W0)
            db0 = torch.empty_like(b0)
            outer_sum_into(dpre1, h, dW0[:, :d], db0)
            outer_sum_into(dpre1, m, dW0[:, d:], None)
            dW3 = torch.empty_like(W3)
            db3 = torch.empty_like(b3)
            # x1 = act(x_hat1 ln1w + ln1b), rebuilt at load time
            outer_sum_into(dpre2, xhat[0], dW3, db3, ctx.act, ln1w, ln1b)
        grads = (dW0, db0, gb1[:d], gb1[d:], dW3, db3, gb2[:d], gb2[d:])
        return ((dh, dm) + sw.deliver(ctx.needs_input_grad, 2,
                                      (W0, b0, ln1w, ln1b, W3, b3, ln2w, ln2b), grads)
                + (None, None, None, None, None, None))


# ----------------------------------------------------------------------------------- 2nd order
# Energy-and-force training (F = -dE/dpos, a loss on F) differentiates the backward pass once
# more.  Inside `with second_order():` the SchNet path records the Functions below instead of the
# once-differentiable ones above: each backward is itself a Function (or plain torch ops), so
# torch.autograd.grad(E, pos, create_graph=True) builds a graph that loss.backward() can walk.
# Outside the context nothing changes.  The other models' Functions stay once-differentiable in
# either state: a second-order backward through them raises.
_SECOND_ORDER = [False]


def second_order_enabled():
    return _SECOND_ORDER[0]


class second_order:
    """Context manager: record twice-differentiable Functions on the SchNet path (CFConv with a
    differentiable cutoff, shifted softplus, the SchNet featurisation, segmented sum / mean,
    gather, ops.linear) and, for a DimeNetPPModel with twice_differentiable=True, on the
    DimeNet++ path (K11 geometry, K18d bases and projection, K19d).  The routing is decided when
    the forward runs; the backward calls may come after the block has exited.  Nests; restores
    the previous state on exit."""

    def __enter__(self):
        if compiling():
            raise NotImplementedError("gmp_amd.second_order() is not supported under "
                                      "torch.compile tracing")
        self.prev = _SECOND_ORDER[0]
        _SECOND_ORDER[0] = True
        return self

    def __exit__(self, *exc):
        _SECOND_ORDER[0] = self.prev
        return False


def _leaf_grad_unused(p):
    """True when p is a leaf whose gradient the running backward pass neither accumulates nor
    captures (torch.autograd.grad(E, pos): the parameters' AccumulateGrad nodes are not part of
    the pass), so an E-sized weight-gradient reduction can be skipped.  The engine refuses the
    query for a leaf that autograd.grad captures: then the gradient is wanted."""
    if p is None or not p.is_leaf:
        return False
    try:
        with torch.enable_grad():
            acc = p.view_as(p).grad_fn.next_functions[0][0]
        return not torch._C._will_engine_execute_node(acc)
    except (RuntimeError, AttributeError, IndexError):
        return False


def _al16(t):
    """Contiguous fp32 at a 16-byte aligned address (a contiguous view at an odd offset is
    copied): what the float4 kernels need."""
    t = _f32c(t)
    return t.clone() if t.data_ptr() % 16 else t


# CFConv is one multilinear form T(g, x, W, C) = sum_e C_e sum_f g[dst_e, f] x[src_e, f] W[e, f].
# Its partial derivatives: over g the receiver aggregate, over x the sender aggregate (the same
# kernel with the index roles swapped: CFAggFn), over W the per-edge product (CFEdgeProdFn), over
# C the per-edge dot product (CFEdgeDotFn).  Every first- and second-order term is one of these
# with arguments substituted, so each Function's backward calls the other two; higher orders
# follow by composition.
#
# Every Function here saves the tensors it was GIVEN, never a contiguous / aligned copy made
# inside forward(): such a copy is cut off from the graph, and a second-order gradient through it
# would silently come out as zero.
class CFAggFn(torch.autograd.Function):
    """out[s] = sum_{e: sidx[e] = s} C[e] x[xidx[e]] * W[e] (K13 over the CSR of sidx); C may be
    None.  The receiver aggregate is (xidx, sidx) = (src, dst), the sender aggregate (dst, src)."""

    @staticmethod
    def forward(ctx, x, W, C, xidx, sidx, n_seg):
        ctx.save_for_backward(x, W, C)
        ctx.xidx, ctx.sidx = xidx, sidx
        return cfconv_aggregate(_al16(x), xidx, _al16(W), _cfconv_csr(sidx, n_seg),
                                None if C is None else _f32c(C))

    @staticmethod
    def backward(ctx, a):
        x, W, C = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = CFAggFn.apply(a, W, C, ctx.sidx, ctx.xidx, x.shape[0]) if need[0] else None
        dW = CFEdgeProdFn.apply(a, x, C, ctx.sidx, ctx.xidx) if need[1] else None
        dC = CFEdgeDotFn.apply(a, x, W, ctx.sidx, ctx.xidx) if C is not None and need[2] else None
        return dx, dW, dC, None, None, None


class CFEdgeProdFn(torch.autograd.Function):
    """out[e] = C[e] g[gidx[e]] * x[xidx[e]] (gmp_cfconv_wgrad_scaled_f32); C may be None."""

    @staticmethod
    def forward(ctx, g, x, C, gidx, xidx):
        ctx.save_for_backward(g, x, C)
        ctx.gidx, ctx.xidx = gidx, xidx
        return _lib.torch_ops().cfconv_wgrad(_al16(g), _i64c(gidx), _al16(x), _i64c(xidx),
                                             None if C is None else _f32c(C))

    @staticmethod
    def backward(ctx, a):
        g, x, C = ctx.saved_tensors
        need = ctx.needs_input_grad
        dg = CFAggFn.apply(x, a, C, ctx.xidx, ctx.gidx, g.shape[0]) if need[0] else None
        dx = CFAggFn.apply(g, a, C, ctx.gidx, ctx.xidx, x.shape[0]) if need[1] else None
        dC = CFEdgeDotFn.apply(g, x, a, ctx.gidx, ctx.xidx) if C is not None and need[2] else None
        return dg, dx, dC, None, None


class CFEdgeDotFn(torch.autograd.Function):
    """out[e] = sum_f g[gidx[e], f] x[xidx[e], f] W[e, f] (gmp_cfconv_cgrad_f32)."""

    @staticmethod
    def forward(ctx, g, x, W, gidx, xidx):
        ctx.save_for_backward(g, x, W)
        ctx.gidx, ctx.xidx = gidx, xidx
        return cfconv_cgrad(_al16(g), gidx, _al16(x), xidx, _al16(W))[0]

    @staticmethod
    def backward(ctx, a):
        g, x, W = ctx.saved_tensors
        need = ctx.needs_input_grad
        dg = CFAggFn.apply(x, W, a, ctx.xidx, ctx.gidx, g.shape[0]) if need[0] else None
        dx = CFAggFn.apply(g, W, a, ctx.gidx, ctx.xidx, x.shape[0]) if need[1] else None
        dW = CFEdgeProdFn.apply(g, x, a, ctx.gidx, ctx.xidx) if need[2] else None
        return dg, dx, dW, None, None


def cfconv_cgrad(g, gidx, x, xidx, w, escale=None):
    """(dc (E), err (1) int32) with dc[e] = sum_f g[gidx[e], f] x[xidx[e], f] w[e, f]
    (* escale[e]) (gmp_cfconv_cgrad_f32); err != 0 when a gather index was out of range."""
    g, x, w = _f32c(g), _f32c(x), _f32c(w)
    _need_cuda(g, x, w)
    return _lib.torch_ops().cfconv_cgrad(g, _i64c(gidx), x, _i64c(xidx), w, escale)


def cfconv_receiver_aggregate(x, W, C, src, dst, n):
    """dT/dg: out[i] = sum_{e: dst[e] = i} C[e] x[src[e]] * W[e] (the CFConv forward)."""
    return CFAggFn.apply(x, W, C, src, dst, n)


def cfconv_sender_aggregate(g, W, C, src, dst, n):
    """dT/dx: out[j] = sum_{e: src[e] = j} C[e] g[dst[e]] * W[e]."""
    return CFAggFn.apply(g, W, C, dst, src, n)


def cfconv_edge_product(g, x, C, src, dst):
    """dT/dW: out[e] = C[e] g[dst[e]] * x[src[e]]."""
    return CFEdgeProdFn.apply(g, x, C, dst, src)


def cfconv_edge_dot(g, x, W, src, dst):
    """dT/dC: out[e] = sum_f g[dst[e], f] x[src[e], f] W[e, f]."""
    return CFEdgeDotFn.apply(g, x, W, dst, src)


class ShiftedSoftplus2Fn(torch.autograd.Function):
    """ShiftedSoftplusFn whose backward is recorded (SspBwdFn)."""

    @staticmethod
    def forward(ctx, x, shift):
        y = _lib.torch_ops().ssp_fwd(x, float(shift))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return SspBwdFn.apply(x, g), None


class SspBwdFn(torch.autograd.Function):
    """dx = g * sigmoid(x) (gmp_ssp_bwd_f32); backward by gmp_ssp_bwd2_f32.  Force training needs
    exactly two orders: the second backward is once-differentiable."""

    @staticmethod
    def forward(ctx, x, g):
        ctx.save_for_backward(x, g)
        return _lib.torch_ops().ssp_bwd(x, _al16(g))

    @staticmethod
    @once_differentiable
    def backward(ctx, a):
        x, g = ctx.saved_tensors
        gg, gx = _lib.torch_ops().ssp_bwd2(x, _al16(g), _al16(a))
        return gx, gg


class EdgeVecToPosFn(torch.autograd.Function):
    """edge_vec_to_pos_grad as a Function: linear in g_vec, its transpose is EdgePosDiffFn."""

    @staticmethod
    def forward(ctx, g_vec, edge_index, n):
        ctx.ei, ctx.n = edge_index, n
        return edge_vec_to_pos_grad(_f32c(g_vec), edge_index, n)

    @staticmethod
    def backward(ctx, a):
        return EdgePosDiffFn.apply(a, ctx.ei), None, None


class EdgePosDiffFn(torch.autograd.Function):
    """a_pos[ei0] - a_pos[ei1] (the gather kernel); its transpose is EdgeVecToPosFn."""

    @staticmethod
    def forward(ctx, a_pos, edge_index):
        ctx.ei, ctx.n = edge_index, a_pos.shape[0]
        a_pos = _f32c(a_pos)
        return gather_rows(a_pos, edge_index[0]) - gather_rows(a_pos, edge_index[1])

    @staticmethod
    def backward(ctx, g):
        return EdgeVecToPosFn.apply(g, ctx.ei, ctx.n), None


class EdgeShiftVectorsFn(torch.autograd.Function):
    """t (E, 3) = S_e . cell[graph_e] with the periodic contract's rounding
    (gmp_edge_shift_vectors_f32); linear in cell, its transpose is EdgeShiftToCellFn."""

    @staticmethod
    def forward(ctx, cell, edge_shift_idx, edge_graph):
        ctx.sidx, ctx.graph, ctx.B = edge_shift_idx, edge_graph, cell.shape[0]
        return _lib.torch_ops().edge_shift_vectors(edge_shift_idx, _f32c(cell), edge_graph)

    @staticmethod
    def backward(ctx, g):
        return EdgeShiftToCellFn.apply(g, ctx.sidx, ctx.graph, ctx.B), None, None


class EdgeShiftToCellFn(torch.autograd.Function):
    """d cell (B, 3, 3) = sum over the edges e of graph b of S_e (x) g_e: the deterministic
    segmented sum over the cached CSR of edge_graph; its transpose is EdgeShiftVectorsFn."""

    @staticmethod
    def forward(ctx, g, edge_shift_idx, edge_graph, B):
        ctx.sidx, ctx.graph = edge_shift_idx, edge_graph
        outer = (edge_shift_idx.to(torch.float32).unsqueeze(2) * _f32c(g).unsqueeze(1))
        out, _ = segment_reduce(outer.reshape(-1, 9), get_csr(edge_graph, B), "sum")
        return out.view(B, 3, 3)

    @staticmethod
    def backward(ctx, a):
        return EdgeShiftVectorsFn.apply(a, ctx.sidx, ctx.graph), None, None, None


def edge_shift_vectors(edge_shift_idx, cell, edge_graph=None):
    """Cartesian shift t (E, 3) of each edge's periodic image (the contract of include/gmp.h,
    K9p) from edge_shift_idx (E, 3) int32, cell (B, 3, 3) and edge_graph (E): the graph of each
    edge, batch[edge_index[1]]; None for a single graph.  Differentiable in cell, to any order."""
    _need_cuda(cell, edge_shift_idx)
    sidx = edge_shift_idx.to(torch.int32).contiguous()
    if edge_graph is None:
        if cell.shape[0] != 1:
            raise ValueError("edge_graph is needed when cell holds more than one graph")
        edge_graph = torch.zeros(sidx.shape[0], dtype=torch.int64, device=sidx.device)
    return EdgeShiftVectorsFn.apply(cell, sidx, _i64c(edge_graph))


class SchNetFeaturize2Fn(torch.autograd.Function):
    """SchNetFeaturizeFn whose backward is recorded (SchNetFeaturizeBwdFn, EdgeVecToPosFn).
    The cotangent of shift (E, 3), if given, is that g_vec."""

    @staticmethod
    def forward(ctx, pos, edge_index, offsets, coeff, cutoff, shift=None):
        ei, off = _i64c(edge_index), _f32c(offsets)
        _need_cuda(pos, ei, off)
        with _timed("edge_featurize"):
            d, rbf, cut = _lib.torch_ops().schnet_featurize(
                _f32c(pos), ei, off, float(coeff), float(cutoff),
                _f32c(shift) if shift is not None else None)
        ctx.save_for_backward(pos, ei, off, shift)
        ctx.coeff, ctx.cutoff = float(coeff), float(cutoff)
        ctx.set_materialize_grads(False)
        return d, rbf, cut

    @staticmethod
    def backward(ctx, g_d, g_rbf, g_cut):
        need_pos, need_shift = ctx.needs_input_grad[0], _needs(ctx, 5)
        if not (need_pos or need_shift) or (g_d is None and g_rbf is None and g_cut is None):
            return None, None, None, None, None, None
        pos, ei, off, shift = ctx.saved_tensors
        g_vec = SchNetFeaturizeBwdFn.apply(pos, ei, off, ctx.coeff, ctx.cutoff, g_d, g_rbf, g_cut,
                                           shift)
        return (EdgeVecToPosFn.apply(g_vec, ei, pos.shape[0]) if need_pos else None, None, None,
                None, None, g_vec if need_shift else None)


class SchNetFeaturizeBwdFn(torch.autograd.Function):
    """g_vec (E, 3) from pos and the cotangents g_d / g_rbf / g_cut (each may be None)
    (gmp_schnet_featurize_bwd_f32); backward by gmp_schnet_featurize_bwd2_f32, whose h_vec goes
    to pos through the segmented sums and, as it is, to shift (E, 3) if given.  The second
    backward is once-differentiable."""

    @staticmethod
    def forward(ctx, pos, ei, off, coeff, cutoff, g_d, g_rbf, g_cut, shift=None):
        ctx.save_for_backward(pos, ei, off, g_d, g_rbf, g_cut, shift)
        ctx.coeff, ctx.cutoff = coeff, cutoff
        opt = [_f32c(t) if t is not None else None for t in (g_d, g_rbf, g_cut)]
        return _lib.torch_ops().schnet_featurize_bwd(
            _f32c(pos), ei, off, coeff, cutoff, *opt, _f32c(shift) if shift is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, a_vec):
        pos, ei, off, *opt, shift = ctx.saved_tensors
        g_d, g_rbf, g_cut = [_f32c(t) if t is not None else None for t in opt]
        need = ctx.needs_input_grad
        need_shift = _needs(ctx, 8)
        want = (g_d is not None and need[5], g_rbf is not None and need[6],
                g_cut is not None and need[7], need[0] or need_shift)
        gg_d, gg_rbf, gg_cut, h_vec = _lib.torch_ops().schnet_featurize_bwd2(
            _f32c(pos), ei, off, ctx.coeff, ctx.cutoff, g_d, g_rbf, g_cut, _f32c(a_vec), *want,
            _f32c(shift) if shift is not None else None)
        dpos = edge_vec_to_pos_grad(h_vec, ei, pos.shape[0]) if need[0] else None
        return (dpos, None, None, None, None, gg_d if want[0] else None,
                gg_rbf if want[1] else None, gg_cut if want[2] else None,
                h_vec if need_shift else None)


class SegmentReduce2Fn(torch.autograd.Function):
    """SegmentReduceFn for sum / mean whose backward is recorded: the gather of g (scaled by
    1 / count for the mean) is SegmentGatherFn, and each is the other's transpose."""

    @staticmethod
    def forward(ctx, src2d, csr, reduce):
        ctx.csr, ctx.reduce, ctx.n = csr, reduce, src2d.shape[0]
        return segment_reduce(src2d, csr, reduce)[0]

    @staticmethod
    def backward(ctx, g):
        return SegmentGatherFn.apply(g, ctx.csr, ctx.reduce, ctx.n), None, None


class SegmentGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, csr, reduce, n_items):
        ctx.csr, ctx.reduce = csr, reduce
        return segment_reduce_bwd(g.contiguous(), csr, reduce, None, n_items)

    @staticmethod
    def backward(ctx, a):
        return SegmentReduce2Fn.apply(a, ctx.csr, ctx.reduce), None, None, None


def segment_reduce_fn(src2d, csr, reduce):
    """The segmented reduce as an autograd Function: twice differentiable for sum / mean inside
    second_order(); max stays once-differentiable."""
    if _SECOND_ORDER[0] and reduce in ("sum", "mean"):
        return SegmentReduce2Fn.apply(src2d, csr, reduce)
    return SegmentReduceFn.apply(src2d, csr, reduce)


class GatherRows2Fn(torch.autograd.Function):
    """GatherRowsFn whose backward (the segmented sum over the CSR of index) is recorded."""

    @staticmethod
    def forward(ctx, src2d, index, n_rows):
        ctx.index, ctx.n_rows = index, n_rows
        return gather_rows(src2d, index)

    @staticmethod
    def backward(ctx, g):
        return SegmentReduce2Fn.apply(g, get_csr(ctx.index, ctx.n_rows), "sum"), None, None


class EdgeLinear2Fn(torch.autograd.Function):
    """EdgeLinearFn whose backward travels through autograd: dx = g W (EdgeDxFn) and (dW, db) =
    (g^T x, colsum g) (EdgeOuterFn) are recorded, with no side stream and no deferred
    accumulation."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W, b)
        return torch.addmm(b, x, W.t()) if b is not None else x.mm(W.t())

    @staticmethod
    def backward(ctx, g):
        x, W, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = EdgeDxFn.apply(g, W) if need[0] else None
        need_w = need[1] and not _leaf_grad_unused(W)
        need_b = b is not None and need[2] and not _leaf_grad_unused(b)
        dW = db = None
        if need_w or need_b:
            dW, db = EdgeOuterFn.apply(g, x)
        return dx, (dW if need_w else None), (db if need_b else None)


class EdgeDxFn(torch.autograd.Function):
    """dx = g W for W (n_out, n_in); backward: dg = a W^T (row GEMM), dW = g^T a (K = rows: the
    deterministic outer sum; the library GEMM inside the op where a shape has no tile bucket).
    Two orders are enough for force training: this backward is once-differentiable."""

    @staticmethod
    def forward(ctx, g, W):
        ctx.save_for_backward(g, W)
        return _dx(g.contiguous(), W)

    @staticmethod
    @once_differentiable
    def backward(ctx, a):
        g, W = ctx.saved_tensors
        need = ctx.needs_input_grad
        dg = torch.nn.functional.linear(a, W) if need[0] else None
        dW = edge_outer_sum_rect(g, a)[0] if need[1] and not _leaf_grad_unused(W) else None
        return dg, dW


class EdgeOuterFn(torch.autograd.Function):
    """(dW, db) = (g^T x, colsum(g)) over the rows (deterministic outer sum); backward: two plain
    row GEMMs, dg = x aW^T + ab, dx = g aW."""

    @staticmethod
    def forward(ctx, g, x):
        ctx.save_for_backward(g, x)
        return edge_outer_sum_rect(g, x)

    @staticmethod
    def backward(ctx, aW, ab):
        g, x = ctx.saved_tensors
        dg = dx = None
        if ctx.needs_input_grad[0]:
            dg = x.mm(aW.t()) if aW is not None else None
            if ab is not None:
                dg = ab.expand(g.shape[0], -1) if dg is None else dg + ab
        if ctx.needs_input_grad[1] and aW is not None:
            dx = g.mm(aW)
        return dg, dx


# ----------------------------------------------------------------------------------- SphereNet
def _pad8(v):
    return (v + 7) // 8 * 8


def _edge_basis_fn(name, family, doc):
    """The autograd Function over gmp.<family>_edge_basis_fwd / _bwd (K18 and K18d take the same
    arguments and return the same shapes)."""

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, dist, freq, zeros, norm, cutoff, envelope_exponent):
            dist, freq = _f32c(dist), _f32c(freq)
            _need_cuda(dist, freq, zeros, norm)
            ctx.save_for_backward(dist, freq, zeros, norm)
            ctx.cutoff, ctx.p = float(cutoff), int(envelope_exponent)
            fwd = getattr(_lib.torch_ops(), family + "_edge_basis_fwd")
            return fwd(dist, freq, zeros, norm, ctx.cutoff, ctx.p)

        @staticmethod
        @once_differentiable
        def backward(ctx, g_rbf, g_jb):
            dist, freq, zeros, norm = ctx.saved_tensors
            g_rbf = _f32c(g_rbf) if g_rbf is not None else None
            g_jb = _f32c(g_jb) if g_jb is not None else None
            bwd = getattr(_lib.torch_ops(), family + "_edge_basis_bwd")
            gd, gf = bwd(dist, freq, zeros, norm, ctx.cutoff, ctx.p, g_rbf, g_jb)
            return gd, gf, None, None, None, None

    Fn.__name__ = Fn.__qualname__ = name
    Fn.__doc__ = doc
    return Fn


SphEdgeBasisFn = _edge_basis_fn(
    "SphEdgeBasisFn", "sph",
    """(rbf (E, k), jb (E, n k)) of K18 gmp_sph_edge_basis_*: the radial basis
    envelope(x) sin(freq x) and the normalised spherical Bessel values N_lq j_l(z_lq x),
    x = dist / cutoff.  Gradients reach dist and freq.""")


def sph_feature_major(weights, width):
    """The first projections of all layers, [(b, F)] * L, as one feature-major (F, pad8(L b))
    matrix with column layer * b + j (the layout K18 reads)."""
    L, b = len(weights), weights[0].shape[0]
    w = torch.stack([_f32c(x) for x in weights]).reshape(L * b, width).t()
    out = w.new_zeros((width, _pad8(L * b)))
    out[:, :L * b] = w
    return out


class SphTripletProjFn(torch.autograd.Function):
    """K18 gmp_sph_triplet_proj_*: S[l] = W_sbf1[l] angle_emb and P[l] = W_t1[l] torsion_emb for
    every layer l at once, the embeddings formed on chip from jb[idx_kj], angle and torsion.
    Returns (S[0], .., S[L-1], P[0], .., P[L-1]).  Gradients: the 2L weights and, where asked
    for, jb (summed per edge over the CSR of idx_kj), angle and torsion."""

    @staticmethod
    def forward(ctx, jb, angle, torsion, idx_kj, pref, n, k, L, *weights):
        jb, angle, torsion = _f32c(jb), _f32c(angle), _f32c(torsion)
        idx_kj = _i64c(idx_kj)
        _need_cuda(jb, angle, torsion, idx_kj, pref, *weights)
        ba, bt = weights[0].shape[0], weights[L].shape[0]
        w1t = sph_feature_major(weights[:L], n * k)
        w2t = sph_feature_major(weights[L:], n * n * k)
        S, P = _lib.torch_ops().sph_triplet_proj_fwd(jb, angle, torsion, idx_kj, pref, w1t, w2t,
                                                     n, k, L, ba, bt)
        ctx.save_for_backward(jb, angle, torsion, idx_kj, pref, w1t, w2t)
        ctx.dims = (n, k, L, ba, bt)
        return tuple(S.unbind(0)) + tuple(P.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        jb, angle, torsion, idx_kj, pref, w1t, w2t = ctx.saved_tensors
        n, k, L, ba, bt = ctx.dims
        T = angle.numel()

        def stacked(gs, b):
            out = jb.new_zeros((L, T, b))
            for l, g in enumerate(gs):
                if g is not None:
                    out[l] = g
            return out

        gS, gP = stacked(grads[:L], ba), stacked(grads[L:], bt)
        geom = any(ctx.needs_input_grad[:3])
        gw1, gw2, gjb_rows, ga, gt = _lib.torch_ops().sph_triplet_proj_bwd(
            jb, angle, torsion, idx_kj, pref, w1t, w2t, n, k, L, ba, bt, gS, gP, geom)
        gjb = None
        if geom and T == 0:
            gjb = torch.zeros_like(jb)
        elif geom:
            gjb, _ = segment_reduce(gjb_rows, get_csr(idx_kj, jb.shape[0]), "sum")
        else:
            ga = gt = None
        gw = [gw1[:, l * ba:(l + 1) * ba].t().contiguous() for l in range(L)]
        gw += [gw2[:, l * bt:(l + 1) * bt].t().contiguous() for l in range(L)]
        return (gjb, ga, gt, None, None, None, None, None) + tuple(gw)


def sph_triplet_embeddings(jb, angle, torsion, idx_kj, pref, n, k):
    """The materialised angle_emb (T, n k) and torsion_emb (T, n^2 k) of K18 (tests and small T;
    the model never forms them)."""
    _need_cuda(jb, angle, torsion, idx_kj, pref)
    return _lib.torch_ops().sph_triplet_emb(_f32c(jb), _f32c(angle), _f32c(torsion),
                                            _i64c(idx_kj), pref, n, k)


def _interact_grad_xd(ctx, interact_fwd, gm, xd, factors, idx_kj, idx_ji):
    """grad_xd of K19 / K19d, where asked for: the forward kernel run over the CSR of idx_kj,
    gathering grad_m by idx_ji.  `factors` are the forward's arguments between src and
    gather_idx."""
    if not ctx.needs_input_grad[0]:
        return None
    if idx_kj.numel() == 0 or xd.shape[0] == 0:
        return torch.zeros_like(xd)
    csr = get_csr(idx_kj, xd.shape[0])
    return interact_fwd(gm, *factors, idx_ji, csr.perm, csr.rowptr)


class TripletInteractFn(torch.autograd.Function):
    """K19 gmp_triplet_interact_*: m[e] = sum over the triplets t of edge e (the contiguous
    range [offsets[e], offsets[e+1]) that K11 emits) of xd[idx_kj[t]] * (W_sbf2 S_t) *
    (W_t2 P_t).  Deterministic both ways; grad_xd runs the same kernel over the CSR of idx_kj."""

    @staticmethod
    def forward(ctx, xd, S, P, Wa, Wt, idx_kj, idx_ji, offsets):
        xd, S, P, Wa, Wt = _f32c(xd), _f32c(S), _f32c(P), _f32c(Wa), _f32c(Wt)
        idx_kj, idx_ji, offsets = _i64c(idx_kj), _i64c(idx_ji), _i64c(offsets)
        _need_cuda(xd, S, P, Wa, Wt, idx_kj, idx_ji, offsets)
        ctx.save_for_backward(xd, S, P, Wa, Wt, idx_kj, idx_ji, offsets)
        return _lib.torch_ops().triplet_interact_fwd(xd, S, P, Wa, Wt, idx_kj, None, offsets)

    @staticmethod
    @once_differentiable
    def backward(ctx, gm):
        xd, S, P, Wa, Wt, idx_kj, idx_ji, offsets = ctx.saved_tensors
        gm = _f32c(gm)
        tops = _lib.torch_ops()
        gS, gP, gWa, gWt = tops.triplet_interact_bwd(gm, xd, S, P, Wa, Wt, idx_kj, offsets)
        gxd = _interact_grad_xd(ctx, tops.triplet_interact_fwd, gm, xd, (S, P, Wa, Wt), idx_kj,
                                idx_ji)
        return gxd, gS, gP, gWa, gWt, None, None, None


# ----------------------------------------------------------------------------------- DimeNet++
DimeEdgeBasisFn = _edge_basis_fn(
    "DimeEdgeBasisFn", "dime",
    """(rbf (E, k), sbe (E, n k)) of K18d gmp_dime_edge_basis_*: env(x) sin(freq x) and
    env(x) N_lq j_l(z_lq x), x = dist / cutoff, env the envelope cut to zero at and beyond the
    cutoff (PyG's [x < 1]).  Gradients reach dist and freq.""")


class DimeTripletProjFn(torch.autograd.Function):
    """K18d gmp_dime_triplet_proj_*: S[l] = W_sbf1[l] sbf for every layer l at once, sbf_t =
    sbe[idx_kj[t]] * Y_l0(angle_t) formed on chip.  Returns (S[0], .., S[L-1]).  Gradients: the
    L weights and, where asked for, sbe (summed per edge over the CSR of idx_kj) and angle."""

    @staticmethod
    def forward(ctx, sbe, angle, idx_kj, pref, n, k, L, *weights):
        sbe, angle, idx_kj = _f32c(sbe), _f32c(angle), _i64c(idx_kj)
        _need_cuda(sbe, angle, idx_kj, pref, *weights)
        b = weights[0].shape[0]
        wt = sph_feature_major(weights, n * k)
        S = _lib.torch_ops().dime_triplet_proj_fwd(sbe, angle, idx_kj, pref, wt, n, k, L, b)
        ctx.save_for_backward(sbe, angle, idx_kj, pref, wt)
        ctx.dims = (n, k, L, b)
        return tuple(S.unbind(0))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        sbe, angle, idx_kj, pref, wt = ctx.saved_tensors
        n, k, L, b = ctx.dims
        T = angle.numel()
        gS = sbe.new_zeros((L, T, b))
        for l, g in enumerate(grads):
            if g is not None:
                gS[l] = g
        geom = any(ctx.needs_input_grad[:2])
        gw, gsbe_rows, ga = _lib.torch_ops().dime_triplet_proj_bwd(sbe, angle, idx_kj, pref, wt,
                                                                   n, k, L, b, gS, geom)
        gsbe = None
        if geom and T == 0:
            gsbe = torch.zeros_like(sbe)
        elif geom:
            gsbe, _ = segment_reduce(gsbe_rows, get_csr(idx_kj, sbe.shape[0]), "sum")
        else:
            ga = None
        gws = [gw[:, l * b:(l + 1) * b].t().contiguous() for l in range(L)]
        return (gsbe, ga, None, None, None, None, None) + tuple(gws)


def dime_triplet_embeddings(sbe, angle, idx_kj, pref, n, k):
    """The materialised sbf (T, n k) of K18d (tests and the composed baseline; the model never
    forms it)."""
    _need_cuda(sbe, angle, idx_kj, pref)
    return _lib.torch_ops().dime_triplet_emb(_f32c(sbe), _f32c(angle), _i64c(idx_kj), pref, n, k)


class TripletInteract1Fn(torch.autograd.Function):
    """K19d gmp_triplet_interact1_*: m[e] = sum over the triplets t of edge e (the contiguous
    range [offsets[e], offsets[e+1]) that K11 emits) of xd[idx_kj[t]] * (W_sbf2 S_t).
    Deterministic both ways; grad_xd runs the same kernel over the CSR of idx_kj."""

    @staticmethod
    def forward(ctx, xd, S, W, idx_kj, idx_ji, offsets):
        xd, S, W = _f32c(xd), _f32c(S), _f32c(W)
        idx_kj, idx_ji, offsets = _i64c(idx_kj), _i64c(idx_ji), _i64c(offsets)
        _need_cuda(xd, S, W, idx_kj, idx_ji, offsets)
        ctx.save_for_backward(xd, S, W, idx_kj, idx_ji, offsets)
        return _lib.torch_ops().triplet_interact1_fwd(xd, S, W, idx_kj, None, offsets)

    @staticmethod
    @once_differentiable
    def backward(ctx, gm):
        xd, S, W, idx_kj, idx_ji, offsets = ctx.saved_tensors
        gm = _f32c(gm)
        tops = _lib.torch_ops()
        gS, gW = tops.triplet_interact1_bwd(gm, xd, S, W, idx_kj, offsets)
        gxd = _interact_grad_xd(ctx, tops.triplet_interact1_fwd, gm, xd, (S, W), idx_kj, idx_ji)
        return gxd, gS, gW, None, None, None


# ------------------------------------------------- DimeNet++, twice differentiable (second_order)
# Energy-and-force training differentiates F = -dE/dpos once more.  Each Function below has the
# forward of its once-differentiable namesake and a backward that is itself a recorded Function
# (*BwdFn), whose backward calls the *_bwd2 kernel and is once-differentiable: exactly two
# orders.  As for CFConv, every Function saves the tensors it was GIVEN.
class DimeEdgeBasis2Fn(torch.autograd.Function):
    """DimeEdgeBasisFn whose backward is recorded (DimeEdgeBasisBwdFn)."""

    @staticmethod
    def forward(ctx, dist, freq, zeros, norm, cutoff, envelope_exponent):
        _need_cuda(dist, freq, zeros, norm)
        ctx.save_for_backward(dist, freq, zeros, norm)
        ctx.cutoff, ctx.p = float(cutoff), int(envelope_exponent)
        ctx.set_materialize_grads(False)
        return _lib.torch_ops().dime_edge_basis_fwd(_f32c(dist), _f32c(freq), zeros, norm,
                                                    ctx.cutoff, ctx.p)

    @staticmethod
    def backward(ctx, g_rbf, g_sbe):
        dist, freq, zeros, norm = ctx.saved_tensors
        if g_rbf is None and g_sbe is None:
            return None, None, None, None, None, None
        gd, gf = DimeEdgeBasisBwdFn.apply(dist, freq, zeros, norm, ctx.cutoff, ctx.p, g_rbf, g_sbe)
        return gd, gf, None, None, None, None


class DimeEdgeBasisBwdFn(torch.autograd.Function):
    """(g_dist, g_freq) from the cotangents g_rbf / g_sbe (each may be None)
    (gmp_dime_edge_basis_bwd_f32); backward by gmp_dime_edge_basis_bwd2_f32."""

    @staticmethod
    def forward(ctx, dist, freq, zeros, norm, cutoff, p, g_rbf, g_sbe):
        ctx.save_for_backward(dist, freq, zeros, norm, g_rbf, g_sbe)
        ctx.cutoff, ctx.p = cutoff, p
        ctx.set_materialize_grads(False)
        opt = [_f32c(t) if t is not None else None for t in (g_rbf, g_sbe)]
        return _lib.torch_ops().dime_edge_basis_bwd(_f32c(dist), _f32c(freq), zeros, norm, cutoff,
                                                    p, *opt)

    @staticmethod
    @once_differentiable
    def backward(ctx, a_dist, a_freq):
        dist, freq, zeros, norm, g_rbf, g_sbe = ctx.saved_tensors
        if a_dist is None and a_freq is None:
            return (None,) * 8
        opt = [_f32c(t) if t is not None else None for t in (g_rbf, g_sbe, a_dist, a_freq)]
        gg_rbf, gg_sbe, h_dist, h_freq = _lib.torch_ops().dime_edge_basis_bwd2(
            _f32c(dist), _f32c(freq), zeros, norm, ctx.cutoff, ctx.p, *opt)
        need = ctx.needs_input_grad
        return (h_dist if need[0] else None, h_freq if need[1] else None, None, None, None, None,
                gg_rbf if g_rbf is not None and need[6] else None,
                gg_sbe if g_sbe is not None and need[7] else None)


def dime_feature_major(weights, width):
    """sph_feature_major from recorded torch ops: the (F, pad8(L b)) matrix stays connected to the
    L weights, so the gradient of a force reaches them."""
    L, b = len(weights), weights[0].shape[0]
    w = torch.cat([x.t() for x in weights], dim=1)
    if w.shape[0] != width:
        raise ValueError(f"dime_feature_major: weights of width {w.shape[0]}, expected {width}")
    pad = _pad8(L * b) - L * b
    return torch.nn.functional.pad(w, (0, pad)) if pad else w.contiguous()


def _sum_rows_per_edge(rows, idx_kj, like):
    if rows.shape[0] == 0:
        return torch.zeros_like(like, dtype=torch.float32)
    return segment_reduce(rows, get_csr(idx_kj, like.shape[0]), "sum")[0]


class DimeTripletProj2Fn(torch.autograd.Function):
    """DimeTripletProjFn on the feature-major weights wt (dime_feature_major) returning the
    stacked S (L, T, b); its backward is recorded (DimeTripletProjBwdFn)."""

    @staticmethod
    def forward(ctx, sbe, angle, wt, idx_kj, pref, n, k, L, b):
        idx_kj = _i64c(idx_kj)
        _need_cuda(sbe, angle, wt, idx_kj, pref)
        ctx.save_for_backward(sbe, angle, wt, idx_kj, pref)
        ctx.dims = (n, k, L, b)
        return _lib.torch_ops().dime_triplet_proj_fwd(_f32c(sbe), _f32c(angle), idx_kj, pref,
                                                      _f32c(wt), n, k, L, b)

    @staticmethod
    def backward(ctx, gS):
        sbe, angle, wt, idx_kj, pref = ctx.saved_tensors
        gw, gsbe, ga = DimeTripletProjBwdFn.apply(sbe, angle, wt, gS, idx_kj, pref, *ctx.dims)
        return gsbe, ga, gw, None, None, None, None, None, None


class DimeTripletProjBwdFn(torch.autograd.Function):
    """(g_wt, g_sbe, g_angle) from gS (L, T, b) (gmp_dime_triplet_proj_bwd_f32 and the per-edge
    sum over the CSR of idx_kj); backward by gmp_dime_triplet_proj_bwd2_f32."""

    @staticmethod
    def forward(ctx, sbe, angle, wt, gS, idx_kj, pref, n, k, L, b):
        ctx.save_for_backward(sbe, angle, wt, gS, idx_kj, pref)
        ctx.dims = (n, k, L, b)
        ctx.set_materialize_grads(False)
        gw, rows, ga = _lib.torch_ops().dime_triplet_proj_bwd(
            _f32c(sbe), _f32c(angle), idx_kj, pref, _f32c(wt), n, k, L, b, _f32c(gS), True)
        return gw, _sum_rows_per_edge(rows, idx_kj, sbe), ga

    @staticmethod
    @once_differentiable
    def backward(ctx, a_wt, a_sbe, a_angle):
        sbe, angle, wt, gS, idx_kj, pref = ctx.saved_tensors
        if a_wt is None and a_sbe is None and a_angle is None:
            return (None,) * 10
        opt = [_f32c(t) if t is not None else None for t in (a_sbe, a_angle, a_wt)]
        need = ctx.needs_input_grad
        geom = need[0] or need[1]
        gg_S, h_wt, h_rows, h_angle = _lib.torch_ops().dime_triplet_proj_bwd2(
            _f32c(sbe), _f32c(angle), idx_kj, pref, _f32c(wt), *ctx.dims, _f32c(gS), *opt, geom)
        h_sbe = _sum_rows_per_edge(h_rows, idx_kj, sbe) if geom else None
        return (h_sbe if need[0] else None, h_angle if need[1] else None,
                h_wt if need[2] else None, gg_S if need[3] else None, None, None, None, None,
                None, None)


# K19d is one trilinear form F(gm, xd, S, W) = sum_t sum_c gm[ji_t, c] xd[kj_t, c] (W S_t)[c]:
# dF/dgm is the message (TripletInteract1_2Fn), dF/dxd the same kernel over the CSR of idx_kj
# (TripletInteract1GradXdFn), (dF/dS, dF/dW) the backward kernel (TripletInteract1BwdFn).  Every
# second-order term is one of these with arguments substituted: composition, no new kernel.
def _i1_msg(xd, S, W, idx_kj, offsets):
    return _lib.torch_ops().triplet_interact1_fwd(_f32c(xd), _f32c(S), _f32c(W), idx_kj, None,
                                                  offsets)


def _i1_grad_xd(gm, S, W, idx_kj, idx_ji, n_edges):
    if idx_kj.numel() == 0 or n_edges == 0:
        return gm.new_zeros((n_edges, W.shape[0]), dtype=torch.float32)
    csr = get_csr(idx_kj, n_edges)
    return _lib.torch_ops().triplet_interact1_fwd(_f32c(gm), _f32c(S), _f32c(W), idx_ji, csr.perm,
                                                  csr.rowptr)


def _i1_bwd(gm, xd, S, W, idx_kj, offsets):
    return _lib.torch_ops().triplet_interact1_bwd(_f32c(gm), _f32c(xd), _f32c(S), _f32c(W),
                                                  idx_kj, offsets)


def _add(a, b):
    return b if a is None else (a if b is None else a + b)


class TripletInteract1_2Fn(torch.autograd.Function):
    """TripletInteract1Fn whose backward is recorded."""

    @staticmethod
    def forward(ctx, xd, S, W, idx_kj, idx_ji, offsets):
        idx_kj, idx_ji, offsets = _i64c(idx_kj), _i64c(idx_ji), _i64c(offsets)
        _need_cuda(xd, S, W, idx_kj, idx_ji, offsets)
        ctx.save_for_backward(xd, S, W, idx_kj, idx_ji, offsets)
        return _i1_msg(xd, S, W, idx_kj, offsets)

    @staticmethod
    def backward(ctx, a):
        xd, S, W, idx_kj, idx_ji, offsets = ctx.saved_tensors
        need = ctx.needs_input_grad
        dxd = dS = dW = None
        if need[0]:
            dxd = TripletInteract1GradXdFn.apply(a, S, W, idx_kj, idx_ji, offsets)
        if need[1] or need[2]:
            dS, dW = TripletInteract1BwdFn.apply(a, xd, S, W, idx_kj, idx_ji, offsets)
        return dxd, (dS if need[1] else None), (dW if need[2] else None), None, None, None


class TripletInteract1GradXdFn(torch.autograd.Function):
    """dF/dxd (E, I) from gm (E, I): the forward kernel over the CSR of idx_kj."""

    @staticmethod
    def forward(ctx, gm, S, W, idx_kj, idx_ji, offsets):
        ctx.save_for_backward(gm, S, W, idx_kj, idx_ji, offsets)
        return _i1_grad_xd(gm, S, W, idx_kj, idx_ji, offsets.numel() - 1)

    @staticmethod
    def backward(ctx, a):
        gm, S, W, idx_kj, idx_ji, offsets = ctx.saved_tensors
        need = ctx.needs_input_grad
        dgm = dS = dW = None
        if need[0]:
            dgm = TripletInteract1_2Fn.apply(a, S, W, idx_kj, idx_ji, offsets)
        if need[1] or need[2]:
            dS, dW = TripletInteract1BwdFn.apply(gm, a, S, W, idx_kj, idx_ji, offsets)
        return dgm, (dS if need[1] else None), (dW if need[2] else None), None, None, None


class TripletInteract1BwdFn(torch.autograd.Function):
    """(dF/dS (T, b), dF/dW (I, b)) from (gm, xd, S, W) (gmp_triplet_interact1_bwd_f32).  Its
    backward reuses the two kernels with (a_S, W) and (S, a_W) substituted and is
    once-differentiable."""

    @staticmethod
    def forward(ctx, gm, xd, S, W, idx_kj, idx_ji, offsets):
        ctx.save_for_backward(gm, xd, S, W, idx_kj, idx_ji, offsets)
        ctx.set_materialize_grads(False)
        return _i1_bwd(gm, xd, S, W, idx_kj, offsets)

    @staticmethod
    @once_differentiable
    def backward(ctx, a_S, a_W):
        gm, xd, S, W, idx_kj, idx_ji, offsets = ctx.saved_tensors
        need = ctx.needs_input_grad
        E = offsets.numel() - 1
        dgm = dxd = dS = dW = None
        for s_, w_ in ((a_S, W), (S, a_W)):
            if s_ is None or w_ is None:
                continue
            if need[0]:
                dgm = _add(dgm, _i1_msg(xd, s_, w_, idx_kj, offsets))
            if need[1]:
                dxd = _add(dxd, _i1_grad_xd(gm, s_, w_, idx_kj, idx_ji, E))
        if a_S is not None and need[3]:
            dW = _i1_bwd(gm, xd, a_S, W, idx_kj, offsets)[1]
        if a_W is not None and need[2]:
            dS = _i1_bwd(gm, xd, S, a_W, idx_kj, offsets)[0]
        return dgm, dxd, dS, dW, None, None, None


class FirstOrderOnlyFn(torch.autograd.Function):
    """Identity whose gradient raises when it is differentiated again (create_graph=True)
    instead of passing as a constant: K11's geometry backward records no graph, and the
    SphereNet path has no second-order kernels."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():  # create_graph=True: the result must not pass as a constant
            g = _NoSecondOrderFn.apply(g.detach().requires_grad_(True))
        return g


class _NoSecondOrderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g):
        return g.view_as(g)

    @staticmethod
    def backward(ctx, a):
        raise RuntimeError("this path is once differentiable: its gradient (e.g. a force) cannot "
                           "be differentiated again")
