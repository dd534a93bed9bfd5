"""fp64 reference of the K8 symmetric contraction (csrc/gmp_sc.hip) on ANY term plan, synthetic
plans that reach the kernels' tile, group and field edges, and the error bound the tests hold the
kernels to.  Pure torch; importable without a GPU.

The polynomial (gmp.h): with xx = [x[b, c, 0..D-1], 1.0],
    out[b, out_base[m] + out_stride[m] c] = sum_{t in row m} coef[t, c] prod_{r < 4} xx[f_r(t)]
    dx[b, c, i]  = sum_t sum_{r : f_r(t) = i} g[b, c, m_t] coef[t, c] prod_{s != r} xx[f_s(t)]
    dcoef[t, c]  = sum_b g[b, c, m_t] prod_{r < 4} xx[f_r(t)]
with g[b, c, m] = gout[b, out_base[m] + out_stride[m] c].

Bound.  Every output element is a recursive fp32 sum of n addends.  To first order the computed sum
differs from the exact one by at most (n - 1 + k) u S, u = 2^-24, S the sum of the addends'
absolute values and k the roundings inside one addend: at most five (the monomial's three
products, g coef, the fma).  bound(n, S) = (n + 8) u S.  S comes from the same evaluation on |x|,
|coef|, |gout| (the derivative of the absolute polynomial with respect to |x_i| or |coef_t| is
exactly the sum of the absolute addends), n is counted from the plan:
    out    the terms of the row
    dx     the factor slots equal to i over all terms (x_i^2 is two addends)
    dcoef  nodes per group + groups (the caller's part.sum(0) belongs to the sum)
An element with no addends has S = 0 and must be exactly 0.0.
"""
import ctypes
import math

import torch

U24 = 2.0 ** -24
ROUTE_FIELDS = ("CT", "npb", "channel_tiles", "node_blocks", "lds_fwd", "lds_dx",
                "CT_d", "terms_per_wg", "z_blocks", "NB", "G", "nodes_per_group")


def route(B, C, D, M, T):
    """gmp_sc_route as a dict (host arithmetic of libgmp.so: the values the launches take)."""
    from gmp_amd import _lib
    out = (ctypes.c_int64 * 12)()
    rc = _lib.load().gmp_sc_route(B, C, D, M, T, out)
    assert rc == 0, rc
    return dict(zip(ROUTE_FIELDS, (int(v) for v in out)))


def out_layout(out_blocks, C):
    """out_base, out_stride of output irreps blocks of widths 2l + 1 (k8_plan's mul_ir layout)."""
    base, stride, m0 = [], [], 0
    for d in out_blocks:
        for mm in range(d):
            base.append(C * m0 + mm)
            stride.append(d)
        m0 += d
    return base, stride


def blocks_for(M):
    """Block widths 1, 3, 5, 7, 9, 11 repeated (the last one cut) to sum M."""
    out, k = [], 0
    while sum(out) < M:
        out.append(min((1, 3, 5, 7, 9, 11)[k % 6], M - sum(out)))
        k += 1
    return out


def make_plan(M, D, C, terms_per_row, out_blocks, seed):
    """A synthetic K8 plan (int32 [row_ptr | out_base | out_stride | terms], the layout of
    gmp_sc.hip's header comment): terms_per_row (an int or one count per row) distinct monomials
    per row of mixed degree 1..4, sorted factors padded with D, about half of them drawn from
    two indices only so that x_i^2, x_i^3 x_j and x_i^4 occur (the dx kernel's product rule takes
    each slot separately); the first and the last non-empty row also hold x_{D-1}^4 and x_0^2.
    Terms of a row ascend by (degree, factors) as k8_plan's do.  Words with m >= 128 are stored
    as negative int32."""
    tpr = [terms_per_row] * M if isinstance(terms_per_row, int) else list(terms_per_row)
    assert len(tpr) == M and sum(out_blocks) == M
    n_mono = math.comb(D + 4, 4) - 1
    assert max(tpr) <= n_mono, "more terms in a row than distinct monomials"
    g = torch.Generator().manual_seed(seed)
    nonempty = [m for m in range(M) if tpr[m] > 0]
    row_ptr, words = [0], []
    for m in range(M):
        monos = set()
        if nonempty and m == nonempty[0]:
            monos.add((D - 1,) * 4)
        if nonempty and m == nonempty[-1] and len(monos) < tpr[m]:
            monos.add((0, 0))
        while len(monos) < tpr[m]:
            nu = int(torch.randint(1, 5, (1,), generator=g))
            if 2 * len(monos) >= n_mono:   # few left (tiny D): any indices
                pool = torch.arange(D)
            elif int(torch.randint(0, 2, (1,), generator=g)):
                pool = torch.randint(0, D, (2,), generator=g)
            else:
                pool = torch.arange(D)
            idx = pool[torch.randint(0, len(pool), (nu,), generator=g)]
            monos.add(tuple(sorted(idx.tolist())))
        for mono in sorted(monos, key=lambda t: (len(t), t)):
            f = list(mono) + [D] * (4 - len(mono))
            words.append(f[0] | f[1] << 6 | f[2] << 12 | f[3] << 18 | m << 24)
        row_ptr.append(len(words))
    base, stride = out_layout(out_blocks, C)
    w = torch.tensor(words, dtype=torch.int64)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)  # int32 bit patterns
    plan = torch.cat([torch.tensor(row_ptr + base + stride, dtype=torch.int64), w])
    return plan.to(torch.int32)


def split_plan(plan, M):
    """row_ptr (M + 1), out_base (M), out_stride (M), factors (T, 4), row (T), all int64."""
    p = plan.detach().cpu().to(torch.int64)
    words = p[3 * M + 1:] & 0xffffffff
    fac = torch.stack([(words >> (6 * r)) & 63 for r in range(4)], 1)
    return p[:M + 1], p[M + 1:2 * M + 1], p[2 * M + 1:3 * M + 1], fac, words >> 24


def _evaluate(plan, M, coef, x, gout, dtype, chunk_elems=1 << 21):
    """out (B, M C), dx (B, C, D), dcoef (T, C) of the plan's polynomial in `dtype`, node chunks of
    about chunk_elems (node, channel, term) triples."""
    B, C, D = x.shape
    _, base, stride, fac, row = split_plan(plan, M)
    T = fac.shape[0]
    col = (base[None, :] + stride[None, :] * torch.arange(C)[:, None])       # (C, M)
    coef_t = coef.to(dtype).t().contiguous()                                   # (C, T)
    rows_1h = torch.zeros(T, M, dtype=dtype)
    rows_1h[torch.arange(T), row] = 1
    slot_1h = []
    for r in range(4):
        h = torch.zeros(T, D + 1, dtype=dtype)
        h[torch.arange(T), fac[:, r]] = 1
        slot_1h.append(h)
    out = torch.zeros(B, M * C, dtype=dtype)
    dx = torch.zeros(B, C, D, dtype=dtype)
    dcoef = torch.zeros(T, C, dtype=dtype)
    step = max(1, chunk_elems // max(1, C * max(T, 1)))
    for b0 in range(0, B, step):
        xb = x[b0:b0 + step].to(dtype)
        nb = xb.shape[0]
        xx = torch.cat([xb, torch.ones(nb, C, 1, dtype=dtype)], -1)
        F = [xx[:, :, fac[:, r]] for r in range(4)]                            # (nb, C, T) each
        mono = (F[0] * F[1]) * (F[2] * F[3])
        out[b0:b0 + nb, col.reshape(-1)] = ((coef_t * mono) @ rows_1h).reshape(nb, C * M)
        gt = gout[b0:b0 + nb].to(dtype)[:, col][:, :, row]                     # (nb, C, T)
        dcoef += (gt * mono).sum(0).t()
        w = gt * coef_t
        others = (F[1] * (F[2] * F[3]), F[0] * (F[2] * F[3]), (F[0] * F[1]) * F[3],
                  (F[0] * F[1]) * F[2])
        acc = torch.zeros(nb, C, D + 1, dtype=dtype)
        for r in range(4):
            acc += (w * others[r]) @ slot_1h[r]
        dx[b0:b0 + nb] = acc[:, :, :D]
    return out, dx, dcoef


def eval_plan64(plan, M, coef, x, gout, n_dcoef=None):
    """fp64 out / dx / dcoef of the plan on the given (fp32 or fp64) values upcast, the absolute
    sums S_* (the same evaluation on absolute values) and the addend counts n_* per element
    (module docstring).  n_dcoef: nodes per group + groups; from gmp_sc_route when not given."""
    B, C, D = x.shape
    row_ptr, base, stride, fac, _ = split_plan(plan, M)
    T = fac.shape[0]
    out, dx, dcoef = _evaluate(plan, M, coef, x, gout, torch.float64)
    S_out, S_dx, S_dcoef = _evaluate(plan, M, coef.abs(), x.abs(), gout.abs(), torch.float64)
    col = (base[None, :] + stride[None, :] * torch.arange(C)[:, None])       # (C, M)
    n_out = torch.zeros(M * C, dtype=torch.float64)
    n_out[col.reshape(-1)] = (row_ptr[1:] - row_ptr[:-1]).double().repeat(C)
    n_dx = torch.bincount(fac.reshape(-1), minlength=D + 1)[:D].double()
    if n_dcoef is None:
        r = route(B, C, D, M, T)
        n_dcoef = r["nodes_per_group"] + r["G"]
    return dict(out=out, dx=dx, dcoef=dcoef, S_out=S_out, S_dx=S_dx, S_dcoef=S_dcoef,
                n_out=n_out, n_dx=n_dx, n_dcoef=float(n_dcoef))


def eval_plan32(plan, M, coef, x, gout):
    """The same polynomial in fp32 on the CPU (sums in the library's order, not the kernels':
    the bound holds for any order)."""
    return _evaluate(plan, M, coef.float(), x.float(), gout.float(), torch.float32)


def bound(n, S):
    """(n + 8) 2^-24 S: derived in the module docstring, not tuned; no test may widen it."""
    return (n + 8.0) * U24 * S


def ratio(got, ref, n, S):
    """max over elements of |got - ref| / bound(n, S); an element with S = 0 counts 0 if it is
    exactly equal and inf otherwise.  n broadcasts against the element shape."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err, bnd = (got - ref).abs(), bound(n, S) * torch.ones_like(ref)
    q = torch.where(bnd > 0, err / bnd.clamp_min(1e-300),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(q.max())


def ratios(ref, out, dx, dcoef):
    """error / bound of the three output families against eval_plan64's dict."""
    return dict(out=ratio(out, ref["out"], ref["n_out"], ref["S_out"]),
                dx=ratio(dx, ref["dx"], ref["n_dx"], ref["S_dx"]),
                dcoef=ratio(dcoef, ref["dcoef"], ref["n_dcoef"], ref["S_dcoef"]))
