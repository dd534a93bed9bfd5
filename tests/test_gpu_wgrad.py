"""Edge outer sums (weight gradients, gmp_wgrad.hip) on the bf16x3-split MFMA path against fp64,
every tiling the rectangular dispatcher picks, the activation prologue, determinism, and the
numerics claim: the split path's error vs fp64 is f32-class — within 3x of the f32-MFMA
kernels' on the same operands (gmp_wgrad_set_f32_mfma switches between them) and no worse than
torch's f32 GEMM.  Second half: every route of the dispatcher at its size thresholds (K = 0,
around 256 and around 262 144; wide m), exactly, on the route the library's query reports."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref(A, B):
    return A.double().t() @ B.double(), A.double().sum(0)


def _err(C, ref, A, B):
    """max |C - ref| / (|A|^T |B|): error relative to the sum of |products| per entry."""
    scale = A.double().abs().t() @ B.double().abs()
    return ((C.double().cpu() - ref) / scale.clamp_min(1e-30)).abs().max().item()


@pytest.mark.parametrize("m,n", [(16, 16), (16, 48), (48, 48), (16, 128), (128, 16), (16, 144),
                                 (48, 144), (128, 48), (128, 80), (128, 128), (128, 144),
                                 (32, 32), (64, 64), (32, 128)])
@pytest.mark.parametrize("K", [5, 4097, 50_021, 300_001, 1_000_003])
def test_outer_sum_split_matches_fp64(m, n, K):
    from gmp_amd import ops
    g = torch.Generator().manual_seed(m * 1000 + n + K)
    A = torch.randn(K, m, generator=g) * torch.rand(K, 1, generator=g)
    B = torch.randn(K, n, generator=g)
    C = torch.empty(m, n, device=DEV)
    cs = torch.empty(m, device=DEV)
    ops.outer_sum_into(A.to(DEV), B.to(DEV), C, cs)
    C2 = torch.empty_like(C)
    ops.outer_sum_into(A.to(DEV), B.to(DEV), C2)
    assert torch.equal(C, C2)  # deterministic
    refC, refs = _ref(A, B)
    assert _err(C, refC, A, B) < 5e-6
    torch.testing.assert_close(cs.cpu().double(), refs, atol=1e-5 * max(1.0, K ** 0.5),
                               rtol=1e-5)


@pytest.mark.parametrize("K", [300_007, 49_999])
def test_outer_sum_strided_blocks(K):
    """column blocks of wider tensors (lda, ldb, ldc > width) on the split path (K = 300k) and
    on the node-level quadrant kernel (K = 50k)"""
    from gmp_amd import ops
    g = torch.Generator().manual_seed(7)
    A = torch.randn(K, 272, generator=g).to(DEV)
    B = torch.randn(K, 200, generator=g).to(DEV)
    C = torch.zeros(300, 260, device=DEV)
    ops.outer_sum_into(A[:, 16:144], B[:, 40:184], C[8:136, 100:244])
    ref = A[:, 16:144].double().t() @ B[:, 40:184].double()
    torch.testing.assert_close(C[8:136, 100:244].double(), ref, atol=2e-3, rtol=1e-5)
    assert C[:8].abs().sum() == 0 and C[:, :100].abs().sum() == 0


@pytest.mark.parametrize("m,n", [(128, 128), (64, 64), (128, 256), (256, 64)])
def test_outer_sum_node_level_quadrants(m, n):
    """Node-level sums (K < 256k rows: the quadrant kernel, outer_sum_quad_kernel) with strided
    operands and output (column blocks of wider tensors) against fp64, colsum included, and
    bitwise determinism."""
    from gmp_amd import ops
    g = torch.Generator().manual_seed(m + n)
    K = 50_003
    A = torch.randn(K, m + 24, generator=g).to(DEV)
    B = torch.randn(K, n + 40, generator=g).to(DEV)
    C = torch.zeros(m + 20, n + 120, device=DEV)
    cs = torch.zeros(m, device=DEV)
    ops.outer_sum_into(A[:, 8:8 + m], B[:, 20:20 + n], C[4:4 + m, 100:100 + n], cs)
    refC, refs = _ref(A[:, 8:8 + m].cpu(), B[:, 20:20 + n].cpu())
    assert _err(C[4:4 + m, 100:100 + n], refC, A[:, 8:8 + m].cpu(), B[:, 20:20 + n].cpu()) < 5e-6
    torch.testing.assert_close(cs.cpu().double(), refs, atol=1e-5 * K ** 0.5, rtol=1e-5)
    assert C[:4].abs().sum() == 0 and C[:, :100].abs().sum() == 0
    C2 = torch.zeros_like(C)
    ops.outer_sum_into(A[:, 8:8 + m], B[:, 20:20 + n], C2[4:4 + m, 100:100 + n])
    assert torch.equal(C, C2)


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_outer_sum_act_prologue(act):
    from gmp_amd import ops
    g = torch.Generator().manual_seed(11)
    K, d = 400_009, 128
    A = torch.randn(K, d, generator=g)
    X = torch.randn(K, d, generator=g)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
    C, cs = ops.edge_outer_sum_act(A.to(DEV), X.to(DEV), w.to(DEV), b.to(DEV), act)
    z = X.double() * w.double() + b.double()
    Y = torch.relu(z) if act == "relu" else z * torch.sigmoid(z)
    refC, refs = _ref(A, Y)
    assert _err(C, refC, A, Y) < 5e-6
    torch.testing.assert_close(cs.cpu().double(), refs, atol=1e-3, rtol=1e-5)


@pytest.mark.parametrize("m,n", [(128, 128), (128, 144), (64, 64)])
def test_split_error_not_above_f32_mfma(m, n):
    """The f32-equivalence claim: same operands through both kernels, error vs fp64."""
    from gmp_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    K = 1_000_000
    A = torch.randn(K, m, generator=g) * torch.rand(K, 1, generator=g)
    B = torch.randn(K, n, generator=g) + 0.5
    refC, _ = _ref(A, B)
    Ad, Bd = A.to(DEV), B.to(DEV)
    errs = {}
    for mode in (1, 0):
        prev = lib.gmp_wgrad_set_f32_mfma(mode)
        try:
            C = torch.empty(m, n, device=DEV)
            ops.outer_sum_into(Ad, Bd, C)
            torch.cuda.synchronize()
        finally:
            lib.gmp_wgrad_set_f32_mfma(prev)
        errs[mode] = _err(C, refC, A, B)
    errs["torch_f32"] = _err(Ad.t() @ Bd, refC, A, B)  # rocBLAS f32 GEMM of the same product
    # f32-class: within 3x of the f32-MFMA split-K kernel and no worse than torch's f32 GEMM
    # (measured: split 1.2e-8, f32 MFMA 5.8e-9 of sum |a b| at 128 x 128; f32 u = 6e-8)
    assert errs[0] <= 3 * errs[1] and errs[0] <= errs["torch_f32"], errs


@pytest.mark.parametrize("m,n1,n2", [(128, 128, 16), (128, 32, 48), (48, 128, 16)])
def test_outer_sum_two_b_operands(m, n1, n2):
    """A^T [B1 | B2] in one pass (gmp_edge_outer_sum_ex2_f32) == the two products side by side"""
    from gmp_amd import ops
    g = torch.Generator().manual_seed(m + n1 + n2)
    K = 400_003
    A = torch.randn(K, m, generator=g)
    B1, B2 = torch.randn(K, n1, generator=g), torch.randn(K, n2 + 8, generator=g)
    Ad, B1d, B2d = A.to(DEV), B1.to(DEV), B2.to(DEV)[:, 4:4 + n2]  # strided second operand
    C = torch.empty(m, n1 + n2, device=DEV)
    cs = torch.empty(m, device=DEV)
    ops.outer_sum_into2(Ad, B1d, B2d, C, cs)
    Bcat = torch.cat([B1, B2[:, 4:4 + n2]], 1)
    refC, refs = _ref(A, Bcat)
    assert _err(C, refC, A, Bcat) < 5e-6
    torch.testing.assert_close(cs.cpu().double(), refs, atol=1e-3, rtol=1e-5)
    # node-level K: outside the split-plane kernel, the op makes two products (same result)
    ops.outer_sum_into2(Ad[:1000], B1d[:1000], B2d[:1000], C, cs)
    refC, refs = _ref(A[:1000], Bcat[:1000])
    assert _err(C, refC, A[:1000], Bcat[:1000]) < 5e-6
    torch.testing.assert_close(cs.cpu().double(), refs, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("d,act,ascale", [(128, "relu", 1.0), (128, "swish", 1e-30),
                                          (64, "swish", 1e20)])
def test_edge_outer_sum_act_hf_vs_fp64(d, act, ascale):
    """The HF weight-gradient outer sum (gmp_edge_outer_sum_act_hf_f32: A scaled by its device
    max word, B = act(X w + b) of LayerNorm rows scaled by sqrt(d) max|w| + max|b|, two fp16
    planes, three products) against fp64 at K = 300k: per entry within 4e-6 of sum |a b|;
    colsum(A) as the x3 kernel's; A scaled by 1e-30 / 1e20 stays exact in relative terms."""
    from gmp_amd import ops
    g = torch.Generator().manual_seed(d)
    K = 300_000
    A = torch.randn(K, d, generator=g) * torch.logspace(-3, 0, d) * ascale
    X = torch.randn(K, d, generator=g)
    X = (X - X.mean(1, keepdim=True)) / X.std(1, unbiased=False, keepdim=True)
    w, b = torch.randn(d, generator=g), torch.randn(d, generator=g) * 0.1
    Ad, Xd, wd, bd = A.to(DEV), X.to(DEV), w.to(DEV), b.to(DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    amax[0] = torch.tensor([A.abs().max().item()]).view(torch.int32)[0]
    C, cs = ops.edge_outer_sum_act(Ad, Xd, wd, bd, act, amax)
    z = X.double() * w.double() + b.double()
    B = torch.relu(z) if act == "relu" else z * torch.sigmoid(z)
    ref = A.double().t() @ B
    mag = A.double().abs().t() @ B.abs()
    err = ((C.cpu().double() - ref).abs() / mag.clamp_min(1e-300)).max().item()
    assert err < 4e-6, err
    cs_ref = A.double().sum(0)
    assert ((cs.cpu().double() - cs_ref).abs() / A.double().abs().sum(0)).max().item() < 1e-6


# ------------------------------------------------------------------ every route, at its thresholds
# Exact tests: operands are integers in [-2, 2] (torch.randint(-2, 3) as f32).  Every product is
# an integer of magnitude <= 4 and every partial sum of K of them is an integer of magnitude
# <= 4 K < 2^24 for K < 4.19 M, so each route is exact whatever its summation order: the three
# bf16 planes (the high plane holds the whole value), the f32 MFMA, the ordered sums of partial
# slabs, the library GEMM.  The comparison is torch.equal against fp64: one dropped, duplicated
# or mis-strided row changes an integer.
from test_wgrad_routes_host import CODE, KS, TABLE  # noqa: E402  (the hand-evaluated routes)

_EXACT_KS = [K for K in KS if K <= 262_145]


def _route_cases():
    cases = []
    for (m, n, lda), rows in TABLE.items():
        if lda != m:
            continue   # the strided rows of the table: test_outer_sum_exact_in_column_blocks
        for K in _EXACT_KS:
            if (m, n) == (1024, 1024) and K > 256:
                continue
            i = KS.index(K)
            cases.append((K, m, n, 0, CODE[rows[0][i]]))
            if rows[1][i] != rows[0][i]:
                cases.append((K, m, n, 1, CODE[rows[1][i]]))
    return cases


_LAST = {}


def _exact_operands(K, m, n):
    """(A, B, A^T B, colsum(A)) for integer operands, the references in fp64 on the device;
    the last triple is kept (the two modes of a shape follow each other)."""
    if _LAST.get("key") != (K, m, n):
        _LAST.clear()
        g = torch.Generator(device=DEV).manual_seed(K * 7 + m * 3 + n)
        A = torch.randint(-2, 3, (K, m), generator=g, device=DEV).float()
        B = torch.randint(-2, 3, (K, n), generator=g, device=DEV).float()
        refC, refs = A.double().t() @ B.double(), A.double().sum(0)
        assert 4 * K < 2 ** 24 and refC.abs().max().item() <= 4 * K
        assert refs.abs().max().item() <= 2 * K
        _LAST.update(key=(K, m, n), val=(A, B, refC, refs))
    return _LAST["val"]


class _wgrad_mode:
    def __init__(self, mode):
        from gmp_amd import _lib
        self.lib, self.mode = _lib.load(), mode

    def __enter__(self):
        self.prev = self.lib.gmp_wgrad_set_f32_mfma(self.mode)
        return self.lib

    def __exit__(self, *exc):
        self.lib.gmp_wgrad_set_f32_mfma(self.prev)


def _route_name(lib, K, m, n, lda, ldb):
    from gmp_amd import _lib
    names = {getattr(_lib, "WGRAD_ROUTE_" + v): v for v in CODE.values() if v != "ARG"}
    return names.get(lib.gmp_edge_outer_sum_ex_route(K, m, n, lda, ldb, -1), "ARG")


@pytest.mark.parametrize("K,m,n,mode,route", _route_cases())
def test_outer_sum_exact_on_every_route(K, m, n, mode, route):
    """ops.outer_sum_into on the route the table names (asserted through the library's query),
    bitwise against fp64; C and colsum start as NaN, so every element is written, by the zero
    fill at K = 0 as well."""
    from gmp_amd import ops
    A, B, refC, refs = _exact_operands(K, m, n)
    C = torch.full((m, n), float("nan"), device=DEV)
    cs = torch.full((m,), float("nan"), device=DEV)
    with _wgrad_mode(mode) as lib:
        assert _route_name(lib, K, m, n, A.stride(0), B.stride(0)) == route
        ops.outer_sum_into(A, B, C, cs)
        torch.cuda.synchronize()
    assert torch.equal(C.double(), refC)
    assert torch.equal(cs.double(), refs)


@pytest.mark.parametrize("K,m,n,mode,route", [
    (0, 128, 144, 0, "ZERO"), (262_144, 128, 144, 0, "X3"), (262_145, 192, 64, 0, "X3"),
    (262_143, 576, 192, 0, "QUAD"), (255, 32, 32, 0, "SQUARE_F32"),
    (262_144, 128, 128, 1, "SQUARE_F32"), (256, 48, 144, 0, "RECT_F32"),
    (262_144, 192, 64, 1, "RECT_F32"), (262_144, 576, 192, 0, "LIBRARY"),
    (0, 576, 192, 0, "LIBRARY"), (1, 272, 16, 0, "LIBRARY")])
def test_outer_sum_exact_in_column_blocks(K, m, n, mode, route):
    """One case per route with A, B, C and colsum as blocks of wider tensors (lda = m + 24,
    ldb = n + 40, ldc = n + 120): the block is exact and the sentinel border is untouched."""
    from gmp_amd import ops
    g = torch.Generator(device=DEV).manual_seed(K + m + n)
    Aw = torch.randint(-2, 3, (K, m + 24), generator=g, device=DEV).float()
    Bw = torch.randint(-2, 3, (K, n + 40), generator=g, device=DEV).float()
    A, B = Aw[:, 8:8 + m], Bw[:, 20:20 + n]
    refC, refs = A.double().t() @ B.double(), A.double().sum(0)
    assert 4 * K < 2 ** 24 and refC.abs().max().item() <= 4 * K
    Cw = torch.full((m + 20, n + 120), 12345.0, device=DEV)
    csw = torch.full((m + 8,), 12345.0, device=DEV)
    wantC, wantcs = Cw.double(), csw.double()
    wantC[4:4 + m, 100:100 + n], wantcs[4:4 + m] = refC, refs
    Cw[4:4 + m, 100:100 + n], csw[4:4 + m] = float("nan"), float("nan")
    with _wgrad_mode(mode) as lib:
        assert _route_name(lib, K, m, n, A.stride(0), B.stride(0)) == route
        ops.outer_sum_into(A, B, Cw[4:4 + m, 100:100 + n], csw[4:4 + m])
        torch.cuda.synchronize()
    assert torch.equal(Cw.double(), wantC)
    assert torch.equal(csw.double(), wantcs)


@pytest.mark.parametrize("K", [0, 262_143, 262_144])
def test_outer_sum_two_b_operands_exact(K):
    """ops.outer_sum_into2 (gmp_edge_outer_sum_ex2_f32) exactly: one split-plane pass at
    K = 262144, two products below it (quadrants for 128 x 128, a bucket for 128 x 16) and two
    zero fills at K = 0; the second operand strided, outputs NaN before the call."""
    from gmp_amd import ops
    m, n1, n2 = 128, 128, 16
    g = torch.Generator(device=DEV).manual_seed(K + 1)
    A = torch.randint(-2, 3, (K, m), generator=g, device=DEV).float()
    B1 = torch.randint(-2, 3, (K, n1), generator=g, device=DEV).float()
    B2 = torch.randint(-2, 3, (K, n2 + 8), generator=g, device=DEV).float()[:, 4:4 + n2]
    refC = A.double().t() @ torch.cat([B1, B2], 1).double()
    assert 4 * K < 2 ** 24 and refC.abs().max().item() <= 4 * K
    C = torch.full((m, n1 + n2), float("nan"), device=DEV)
    cs = torch.full((m,), float("nan"), device=DEV)
    with _wgrad_mode(0) as lib:
        want = "X3" if K >= 262_144 else ("QUAD" if K else "ZERO")
        assert _route_name(lib, K, m, n1, m, n1) == want
        if K >= 262_144:
            assert _route_name(lib, K, m, n1 + n2, m, n1 + n2) == "X3"
        ops.outer_sum_into2(A, B1, B2, C, cs)
        torch.cuda.synchronize()
    assert torch.equal(C.double(), refC)
    assert torch.equal(cs.double(), A.double().sum(0))


def _err_dev(C, A, B):
    """_err with everything on the device"""
    ref = A.double().t() @ B.double()
    scale = A.double().abs().t() @ B.double().abs()
    return ((C.double() - ref) / scale.clamp_min(1e-30)).abs().max().item()


@pytest.mark.parametrize("m,n", [(128, 128), (128, 144), (576, 192)])
@pytest.mark.parametrize("K", [262_143, 262_144])
def test_outer_sum_random_values_at_the_split_threshold(K, m, n):
    """Random-valued operands either side of kX3MinK at the file's 5e-6 of sum |a b|; where the
    route is the library GEMM (576 x 192 at K = 262144) the op's result is only held to be no
    worse than A.t() @ B on the same device: the same product, the test is about routing."""
    from gmp_amd import ops
    g = torch.Generator(device=DEV).manual_seed(K + m + n)
    A = torch.randn(K, m, generator=g, device=DEV) * torch.rand(K, 1, generator=g, device=DEV)
    B = torch.randn(K, n, generator=g, device=DEV)
    C = torch.full((m, n), float("nan"), device=DEV)
    cs = torch.full((m,), float("nan"), device=DEV)
    with _wgrad_mode(0) as lib:
        route = _route_name(lib, K, m, n, m, n)
        ops.outer_sum_into(A, B, C, cs)
        torch.cuda.synchronize()
    want = {262_143: "QUAD" if m % 64 == 0 and n % 64 == 0 else "RECT_F32",
            262_144: "LIBRARY" if m > 256 else "X3"}[K]
    assert route == want
    err = _err_dev(C, A, B)
    print(f"K={K} {m}x{n} {route}: err {err:.3e}")
    if route == "LIBRARY":
        assert err <= _err_dev(A.t() @ B, A, B)
    else:
        assert err < 5e-6
    torch.testing.assert_close(cs.double(), A.double().sum(0), atol=1e-5 * K ** 0.5, rtol=1e-5)
