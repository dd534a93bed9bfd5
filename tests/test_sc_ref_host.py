"""Host-side checks of the K8 reference and validator (no GPU): tests/sc_ref.py's fp64 evaluator
equals the per-irrep contraction in double on real modules, its bound rejects every single-entry
mutation of a plan evaluated in fp32, equivariant.check_k8_plan accepts what k8_plan and
sc_ref.make_plan build and rejects one violation of each of its rules."""
import ctypes
import functools
import os

import pytest
import torch

import sc_ref


def _eq():
    from gmp_amd import equivariant
    return equivariant


def _dims(irr):
    C = int(irr.split("x")[0])
    return C, sum(2 * int(t.split("x")[1][:-1]) + 1 for t in irr.split("+"))


@pytest.mark.parametrize("irr,corr", [("3x0e+3x1o+3x2e", 3), ("2x0e+2x1o", 4)])
def test_eval_plan64_equals_contraction_in_double(irr, corr):
    """eval_plan64 on the module's own plan and k8_coefficients() against the per-irrep
    Contraction path in double: out, dx and the weight gradients pulled back through
    k8_coefficients, to 1e-12 of each array's scale."""
    eq = _eq()
    torch.manual_seed(10 + corr)
    sc = eq.SymmetricContraction(irr, irr, corr).double()
    assert sc._k8
    C, D = _dims(irr)
    M = sc._k8_rows
    x = torch.randn(23, C, D, dtype=torch.float64, requires_grad=True)
    gout = torch.randn(23, M * C, dtype=torch.float64)
    y = torch.cat([c(x) for c in sc.contractions.values()], dim=-1)
    (y * gout).sum().backward()
    want = {k: p.grad.clone() for k, p in sc.named_parameters()}
    sc.zero_grad(set_to_none=True)
    coef = sc.k8_coefficients()
    ref = sc_ref.eval_plan64(sc._k8_plan, M, coef.detach(), x.detach(), gout, n_dcoef=24)
    coef.backward(ref["dcoef"])

    def close(a, b, name):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), name
    close(ref["out"], y.detach(), "out")
    close(ref["dx"], x.grad, "dx")
    for k, p in sc.named_parameters():
        close(p.grad, want[k], k)


# ------------------------------------------------------------------------- mutation sensitivity
_MUT = dict(M=9, D=5, C=3, B=16, tpr=[0, 3, 7, 1, 5, 0, 9, 2, 6], blocks=[1, 3, 5])


@functools.lru_cache(maxsize=None)
def _mut_case():
    c = _MUT
    plan = sc_ref.make_plan(c["M"], c["D"], c["C"], c["tpr"], c["blocks"], seed=4)
    _eq().check_k8_plan(plan, c["M"], c["D"], c["C"])
    g = torch.Generator().manual_seed(5)
    T = sum(c["tpr"])
    coef = torch.randn(T, c["C"], generator=g)
    x = torch.randn(c["B"], c["C"], c["D"], generator=g)
    gout = torch.randn(c["B"], c["M"] * c["C"], generator=g)
    ref = sc_ref.eval_plan64(plan, c["M"], coef, x, gout, n_dcoef=c["B"] + 1)
    return plan, coef, x, gout, ref


def _caught(plan, coef):
    """Whether the fp32 evaluation of (plan, coef) breaks the bound of the clean reference on at
    least one element of out."""
    _, _, x, gout, ref = _mut_case()
    out, dx, dcoef = sc_ref.eval_plan32(plan, _MUT["M"], coef, x, gout)
    return sc_ref.ratio(out, ref["out"], ref["n_out"], ref["S_out"]) > 1.0


def test_bound_holds_for_the_clean_fp32_walk():
    plan, coef, x, gout, ref = _mut_case()
    r = sc_ref.ratios(ref, *sc_ref.eval_plan32(plan, _MUT["M"], coef, x, gout))
    print("clean fp32 error / bound:", r)
    assert max(r.values()) < 1.0, r


def test_bound_catches_every_single_mutation():
    """Every single-term mutation of the plan (each term dropped; each term's first factor index
    off by one; each term's channel-0 coefficient taken from channel 1; each pair of adjacent
    rows' output columns swapped) breaks bound on at least one element of out."""
    plan, coef, _, _, _ = _mut_case()
    M, D = _MUT["M"], _MUT["D"]
    T = coef.shape[0]
    row_ptr = plan[:M + 1].clone()
    missed = []
    for t in range(T):
        # dropped: the term and its coefficient leave, later rows move up
        m = int((plan[3 * M + 1 + t].long() & 0xffffffff) >> 24)
        p = torch.cat([plan[:3 * M + 1 + t], plan[3 * M + 2 + t:]])
        p[m + 1:M + 1] -= 1
        if not _caught(p, torch.cat([coef[:t], coef[t + 1:]])):
            missed.append(("drop", t))
        # factor off by one (a padding slot D becomes x_{D-1})
        p = plan.clone()
        w = int(p[3 * M + 1 + t].long() & 0xffffffff)
        f0 = w & 63
        w = (w & ~63) | ((f0 + 1) % D if f0 < D else D - 1)
        p[3 * M + 1 + t] = w - (1 << 32) if w >= (1 << 31) else w
        if not _caught(p, coef):
            missed.append(("factor", t))
        # neighbouring channel's coefficient
        cf = coef.clone()
        cf[t, 0] = coef[t, 1]
        if not _caught(plan, cf):
            missed.append(("channel", t))
    assert int(row_ptr[M]) == T
    for m in range(M - 1):
        if row_ptr[m + 1] == row_ptr[m] and row_ptr[m + 2] == row_ptr[m + 1]:
            continue  # two empty rows: both columns are 0.0 either way
        p = plan.clone()
        for off in (M + 1, 2 * M + 1):  # out_base and out_stride travel together
            p[off + m], p[off + m + 1] = plan[off + m + 1], plan[off + m]
        if not _caught(p, coef):
            missed.append(("column", m))
    n = 3 * T + M - 1
    print(f"mutations caught: {n - len(missed)} of {n}")
    assert not missed, missed


# --------------------------------------------------------------------------------------- route
def test_route_query_on_the_host():
    """gmp_sc_route is host arithmetic (no device needed).  The expected values are worked out
    by hand from the launch code as it stood before the query existed (node blocks, which depend
    on the device's CU count, are left to the GPU tests)."""
    from gmp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmp.so not built")
    r = sc_ref.route(100, 3, 4, 4, 20)
    assert (r["CT"], r["npb"], r["channel_tiles"]) == (3, 85, 1)
    assert (r["lds_fwd"], r["lds_dx"]) == (256 * 5 * 4, 2 * 256 * 5 * 4)
    r = sc_ref.route(64, 16, 63, 9, 120)
    assert (r["CT"], r["npb"], r["lds_fwd"], r["lds_dx"]) == (16, 16, 66_560, 133_120)
    r = sc_ref.route(100, 33, 9, 9, 60)
    assert (r["CT"], r["channel_tiles"]) == (16, 3)
    for T, ctd, tpb, zb in ((1, 16, 256, 1), (256, 16, 256, 1), (257, 15, 273, 1),
                            (273, 15, 273, 1), (274, 14, 292, 1), (586, 6, 682, 1)):
        r = sc_ref.route(70, 17, 9, 9, T)
        assert (r["CT_d"], r["terms_per_wg"], r["z_blocks"]) == (ctd, tpb, zb), (T, r)
    r = sc_ref.route(40, 3, 16, 16, 4096)
    assert (r["CT_d"], r["terms_per_wg"], r["z_blocks"]) == (1, 4096, 1)
    r = sc_ref.route(40, 3, 16, 16, 4097)
    assert (r["CT_d"], r["terms_per_wg"], r["z_blocks"]) == (1, 4096, 2)
    assert sc_ref.route(40, 16, 63, 255, 255)["NB"] == 3      # 16384 // (16 * 319)
    assert sc_ref.route(40, 4, 4, 4, 16)["NB"] == 32
    for B, G, per in ((0, 1, 0), (1, 1, 1), (256, 1, 256), (257, 2, 129), (32_768, 128, 256),
                      (32_769, 128, 257), (33_000, 128, 258)):
        r = sc_ref.route(B, 4, 4, 4, 16)
        assert (r["G"], r["nodes_per_group"]) == (G, per), (B, r)
    assert sc_ref.route(40, 4, 4, 4, 0)["z_blocks"] == 0      # T = 0: dcoef is not launched
    out = (ctypes.c_int64 * 12)()
    lib = _lib.load()
    for bad in ((-1, 4, 4, 4, 1), (1, 0, 4, 4, 1), (1, 4, 64, 4, 1), (1, 4, 0, 4, 1),
                (1, 4, 4, 256, 1), (1, 4, 4, 0, 1), (1, 4, 4, 4, -1)):
        assert lib.gmp_sc_route(*bad, out) == _lib.GMP_ERR_ARG, bad


# ----------------------------------------------------------------------------------- validator
@pytest.mark.parametrize("irr,corr", [("3x0e+3x1o+3x2e", 3), ("2x0e+2x0o+2x1e+2x1o+2x2e+2x2o", 3),
                                      ("2x0e+2x1o+2x2e+2x3o+2x4e+2x5o", 2), ("2x0e+2x1o", 4),
                                      ("2x1o+2x0e+2x1e", 2)])
def test_check_k8_plan_accepts_module_plans(irr, corr):
    """The plans of tests/test_equivariant_host.py::test_k8_term_plan_matches_contraction."""
    eq = _eq()
    sc = eq.SymmetricContraction(irr, irr, corr)
    assert sc._k8
    C, D = _dims(irr)
    eq.check_k8_plan(sc._k8_plan, sc._k8_rows, D, C)


@pytest.mark.parametrize("M,D,C,tpr,seed", [
    (4, 4, 3, 5, 0), (9, 9, 17, [0, 7, 7, 7, 0, 7, 7, 7, 0], 1), (2, 1, 4, 4, 2),
    (255, 9, 4, [1, 2, 3] * 85, 3), (255, 63, 16, 1, 4), (9, 63, 16, 13, 5), (4, 4, 4, 0, 6),
    (16, 16, 3, [257] + [256] * 15, 7)])
def test_make_plan_passes_check(M, D, C, tpr, seed):
    plan = sc_ref.make_plan(M, D, C, tpr, sc_ref.blocks_for(M), seed)
    _eq().check_k8_plan(plan, M, D, C)
    row_ptr, _, _, fac, row = sc_ref.split_plan(plan, M)
    T = int(row_ptr[M])
    assert plan.dtype == torch.int32 and plan.numel() == 3 * M + 1 + T
    assert bool((fac[:, :-1] <= fac[:, 1:]).all())          # sorted, padding D last
    if M > 128 and T:
        assert bool((plan[3 * M + 1:][row >= 128] < 0).all())  # the sign bit, as k8_plan stores
    if T >= 8 and D > 1:
        deg = (fac < D).sum(1)
        assert set(deg.tolist()) == {1, 2, 3, 4}
        assert bool(((fac[:, :-1] == fac[:, 1:]) & (fac[:, 1:] < D)).any())  # a repeated factor


def _good():
    M, D, C = 4, 4, 3
    return sc_ref.make_plan(M, D, C, [2, 0, 3, 1], [1, 3], seed=9), M, D, C


@pytest.mark.parametrize("rule", ["row_ptr0", "row_ptr_decreasing", "row_ptr_end", "row_field",
                                  "factor", "rows_cap", "dim_cap", "columns_overlap",
                                  "columns_outside", "short", "dtype"])
def test_check_k8_plan_rejects(rule):
    eq = _eq()
    plan, M, D, C = _good()
    eq.check_k8_plan(plan, M, D, C)
    p, T0 = plan.clone(), 3 * M + 1
    if rule == "row_ptr0":
        p[0] = 1
    elif rule == "row_ptr_decreasing":
        p[1], p[2] = 3, 2          # 0 3 2 5 6
    elif rule == "row_ptr_end":
        p[M] = 7                   # one past the terms the plan holds
    elif rule == "row_field":
        p[T0] = int(p[T0]) + (1 << 24)
    elif rule == "factor":
        p[T0] = (int(p[T0]) & ~63) | (D + 1)
    elif rule == "rows_cap":
        big = sc_ref.make_plan(256, D, C, 0, sc_ref.blocks_for(256), 0)
        with pytest.raises(ValueError):
            eq.check_k8_plan(big, 256, D, C)
        return
    elif rule == "dim_cap":
        with pytest.raises(ValueError):
            eq.check_k8_plan(plan, M, 64, C)
        return
    elif rule == "columns_overlap":
        p[M + 1 + 1] = p[M + 1 + 2]          # two rows of the 1o block on one column
    elif rule == "columns_outside":
        p[M + 1 + 3] = int(p[M + 1 + 3]) + C * M
    elif rule == "short":
        p = p[:3 * M]
    elif rule == "dtype":
        p = p.long()
    with pytest.raises(ValueError):
        eq.check_k8_plan(p, M, D, C)
