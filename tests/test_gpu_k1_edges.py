"""K1 (csrc/gmp_featurize.hip: featurize_fwd_kernel, featurize_bwd_kernel) at the raw per-edge
ops torch.ops.gmp.edge_featurize{,_bwd,_gvp,_gvp_bwd} against the fp64 oracle (tests/k1_ref.py),
edge by edge: random edges from r = 1e-6 to 1.5 r_max, edges on the axes, face and body diagonals
and a hair off an axis, edges at, one ulp inside, one ulp outside and far past the cutoff,
zero-length edges and a true self-loop; lmax 0..5, num_bessel 0, 1, 8, 32 (33 raises), p 2, 5, 6;
random, radial (g_sh = c Y) and one-hot cotangents; the GVP variant; the shifted entry; a second
trip of the grid-stride loop; the scatter to pos.

Every edge is isolated (k1_ref.isolated_graph: pos[2e] = vec_e, pos[2e + 1] = 0), so the kernel's
vector is exactly the chosen fp32 one and nothing is summed between the kernel and the check.
Bounds: |got - ref64| <= K 2^-24 scale per entry (forward) or per edge (g_vec), the scales of
k1_ref's docstring, K = 4 max(U_ref, 1) with U_ref the fp32 oracle's own worst error in the same
units on the same inputs (k1_ref.kernel_bound).  Exact where stated.  Every test prints its
figures (kernel, U_ref, bound) before it asserts."""
import pytest
import torch

import k1_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from gmp_amd import _lib
    return _lib.torch_ops()


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _is_zero(x, signed=False):
    """All bits zero (+0.0); signed=True also takes -0.0 (the product of a negative Bessel factor
    and the zero cutoff, as the reference's own radial block gives)."""
    b = _bits(x)
    return bool(((b & 0x7fffffff) == 0).all()) if signed else bool((b == 0).all())


def _graph(vec, self_loop=True):
    pos, ei = k1_ref.isolated_graph(vec, self_loop_last=self_loop)
    return pos.to(DEV), ei.to(DEV)


def _d(t):
    return None if t is None else t.to(DEV)


def _run(c, vec=None, shift=None, pos_ei=None):
    """sh, rad and the three backward combinations (g_sh only, g_rad only, both) of the
    equivariant ops, on the case's isolated edges."""
    vec = c.vec if vec is None else vec
    g_sh, g_rad, _ = c.cots
    pos, ei = pos_ei if pos_ei is not None else _graph(vec)
    o = _ops()
    sh, rad = o.edge_featurize(pos, ei, *c.consts, c.lmax, shift)
    out = dict(sh=sh, rad=rad)
    out["gv_sh"] = o.edge_featurize_bwd(pos, ei, *c.consts, _d(g_sh), None, c.lmax, shift)
    out["gv_rad"] = o.edge_featurize_bwd(pos, ei, *c.consts, None, _d(g_rad), c.lmax, shift)
    out["gv_both"] = o.edge_featurize_bwd(pos, ei, *c.consts, _d(g_sh), _d(g_rad), c.lmax, shift)
    torch.cuda.synchronize()
    E = vec.shape[0]
    assert sh.shape == (E, (c.lmax + 1) ** 2) and rad.shape == (E, len(c.consts[0]))
    assert all(out[k].shape == (E, 3) for k in ("gv_sh", "gv_rad", "gv_both"))
    return out


def _hold(tag, c, got, keys, rows=None):
    """Print kernel / U_ref / bound per quantity, then assert kernel <= 4 max(U_ref, 1)."""
    u_ref = c.u_ref
    q = k1_ref.compare({k: got[k].cpu() for k in keys}, c.vec, c.blk, c.lmax, c.cots, c.ref, rows)
    bad = []
    for k in keys:
        b = k1_ref.kernel_bound(u_ref[k])
        print(f"K1 {tag}: {k:8s} kernel {q[k]:7.2f} units  U_ref {u_ref[k]:5.2f}  bound {b:6.2f}")
        if not q[k] <= b:
            bad.append((k, q[k], b))
    assert not bad, (tag, bad)
    return q


def _zero_length_rows(c, got):
    """vec = 0 and the self-loop (a, a): what the reference's forward gives, exact zeros back."""
    z = c.cls["zero"]
    if "sh" in got:
        want = torch.zeros(len(z), (c.lmax + 1) ** 2)
        want[:, 0] = 1.0
        assert torch.equal(got["sh"][z].cpu(), want)
    assert bool(torch.isnan(got["rad"][z]).all())
    if "unit" in got:
        assert _is_zero(got["unit"][z])
    for k in ("gv_sh", "gv_rad", "gv_unit", "gv_both"):
        if k in got:
            assert _is_zero(got[k][z]), k


def _past_cutoff_rows(c, got):
    """Every edge past the cutoff (not only the structured ones): exact zeros."""
    past = c.vec.double().norm(dim=-1) > c.consts[2] * (1 + 1e-6)
    assert int(past.sum()) > 100
    assert _is_zero(got["rad"][past], signed=True) and _is_zero(got["gv_rad"][past])
    if "gv_sh" in got:
        assert _same_bits(got["gv_both"][past], got["gv_sh"][past])


def _joint(c, got, a, b, both):
    """The two single-cotangent runs sum to the joint run within the joint run's bound (in the
    kernel the joint result is the fp32 sum of the two parts)."""
    sc = k1_ref.scales(c.vec, c.blk, c.lmax, *c.cots)
    rows = k1_ref.live_rows(c.vec)
    bound = k1_ref.U24 * (k1_ref.kernel_bound(c.u_ref[a]) * sc[a]
                          + k1_ref.kernel_bound(c.u_ref[b]) * sc[b])
    err = (got[a].cpu().double() + got[b].cpu().double() - got[both].cpu().double()).norm(dim=-1)
    assert bool((err[rows] <= bound[rows]).all()), float((err[rows] / bound[rows]).max())
    ref = c.ref[a] + c.ref[b]
    err = (got[both].cpu().double() - ref).norm(dim=-1)
    print(f"K1 joint {a}+{b}: worst error / bound {float((err[rows] / bound[rows]).max()):.3f}")
    assert bool((err[rows] <= bound[rows]).all())


# ------------------------------------------------------------------------------------- lmax sweep
@pytest.mark.parametrize("lmax,r_max,nb,p", k1_ref.CASES_LMAX)
def test_lmax_vs_fp64(lmax, r_max, nb, p):
    c = k1_ref.case(lmax, r_max, nb, p, "random")
    got = _run(c)
    _zero_length_rows(c, got)
    _past_cutoff_rows(c, got)
    _hold(f"lmax={lmax}", c, got, ("sh", "rad", "gv_sh", "gv_rad"))
    _joint(c, got, "gv_sh", "gv_rad", "gv_both")
    if lmax == 0:
        assert bool((got["sh"] == 1.0).all())
        assert _is_zero(got["gv_sh"])
        assert _same_bits(got["gv_both"], got["gv_rad"])


def test_cutoff_edges():
    """r == r_max, one ulp inside, one ulp outside, 2 r_max, on every axis: the radial rows and
    the radial part of g_vec are exact zeros at and past r_max (the rows as signed zeros, the
    gradient +0.0), finite and within the bound just inside; the SH part does not stop there."""
    c = k1_ref.case(5, 2.0, 8, 5, "random")
    r_max = c.consts[2]
    r = c.vec.double().norm(dim=-1)
    at, inside, out = c.cls["cut_at"], c.cls["cut_in"], c.cls["cut_out"]
    assert bool((r[at] == r_max).all()) and bool((r[inside] < r_max).all())
    assert bool((r[out] > r_max).all())
    assert float((r_max - r[inside]).max()) <= 2.0 ** -22 * r_max
    got = _run(c)
    for rows in (at, out):
        assert _is_zero(got["rad"][rows], signed=True)
        assert _is_zero(got["gv_rad"][rows])
        assert _same_bits(got["gv_both"][rows], got["gv_sh"][rows])
        assert bool((got["gv_sh"][rows].norm(dim=-1) > 0).all())
    assert bool(torch.isfinite(got["rad"][inside]).all())
    assert bool(torch.isfinite(got["gv_rad"][inside]).all())
    for name in ("cut_at", "cut_in", "cut_out"):
        _hold(name, c, got, ("sh", "rad", "gv_sh", "gv_rad"), rows=c.cls[name])
    # the same through the GVP entry
    o = _ops()
    pos, ei = _graph(c.vec)
    rad, unit = o.edge_featurize_gvp(pos, ei, *c.consts)
    gv = o.edge_featurize_gvp_bwd(pos, ei, *c.consts, c.cots[1].to(DEV), None)
    for rows in (at, out):
        assert _is_zero(rad[rows], signed=True) and _is_zero(gv[rows])


# --------------------------------------------------------------------------- radial parameters
@pytest.mark.parametrize("lmax,r_max,nb,p", k1_ref.CASES_RADIAL)
def test_radial_parameters_vs_fp64(lmax, r_max, nb, p):
    c = k1_ref.case(lmax, r_max, nb, p, "random")
    got = _run(c)
    _zero_length_rows(c, got)
    _past_cutoff_rows(c, got)
    _hold(f"nb={nb} p={p}", c, got, ("sh", "rad", "gv_sh", "gv_rad"))
    _joint(c, got, "gv_sh", "gv_rad", "gv_both")
    for rows in (c.cls["cut_at"], c.cls["cut_out"]):
        assert _is_zero(got["rad"][rows], signed=True) and _is_zero(got["gv_rad"][rows])


def test_num_bessel_0_and_33():
    """nb = 0: an empty radial tensor and an SH-only gradient; nb = 33 (> kMaxBessel) raises."""
    c = k1_ref.case(2, 3.7, 0, 5, "random")
    got = _run(c)
    assert got["rad"].shape == (c.vec.shape[0], 0)
    assert _is_zero(got["gv_rad"])
    assert _same_bits(got["gv_both"], got["gv_sh"])
    _hold("nb=0", c, got, ("sh", "gv_sh"))
    o = _ops()
    pos, ei = _graph(c.vec[:8], self_loop=False)
    w33 = [0.1 * (n + 1) for n in range(33)]
    with pytest.raises(RuntimeError):
        o.edge_featurize(pos, ei, w33, 1.0, 3.7, 5.0, 2, None)
    with pytest.raises(RuntimeError):
        o.edge_featurize_bwd(pos, ei, w33, 1.0, 3.7, 5.0, None, torch.zeros(8, 33, device=DEV), 2,
                             None)
    with pytest.raises(RuntimeError):
        o.edge_featurize_gvp(pos, ei, w33, 1.0, 3.7, 5.0)
    with pytest.raises(RuntimeError):
        o.edge_featurize_gvp_bwd(pos, ei, w33, 1.0, 3.7, 5.0, torch.zeros(8, 33, device=DEV), None)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------- cotangents
def test_radial_cotangent_projection():
    """g_sh = c_e Y(vec_e): the fp64 g_vec is ~0, so the kernel's g_vec is all error; a missing
    - u (u . du) projection leaves (1/r) sum_l l c |Y_l|^2 there, thousands of units."""
    c = k1_ref.case(5, 2.0, 8, 5, "radial")
    got = _run(c)
    _zero_length_rows(c, got)
    _hold("radial cotangent", c, got, ("gv_sh",))
    for name in ("axis", "face", "body", "near_axis", "cut_at"):
        _hold(f"radial cotangent, {name}", c, got, ("gv_sh",), rows=c.cls[name])


@pytest.mark.parametrize("kind", ["onehot", "onehot_tiled"])
def test_onehot_cotangents(kind):
    """One column of the SH Jacobian per edge: column e mod 36 over the whole edge set, and every
    column on every structured direction (axis, face and body diagonals, a hair off an axis),
    where most terms of the l = 4, 5 recursion vanish."""
    c = k1_ref.case(5, 2.0, 8, 5, kind)
    got = _run(c, pos_ei=_graph(c.vec, self_loop="zero" in c.cls))
    if "zero" in c.cls:
        _zero_length_rows(c, got)
    _hold(kind, c, got, ("sh", "gv_sh"))
    for name in ("axis", "face", "body", "near_axis"):
        _hold(f"{kind}, {name}", c, got, ("sh", "gv_sh"), rows=c.cls[name])


# ------------------------------------------------------------------------------------------ GVP
@pytest.mark.parametrize("r_max,nb,p", [(2.0, 8, 5), (3.7, 32, 5)])
def test_gvp_variant_vs_fp64(r_max, nb, p):
    """edge_featurize_gvp and its backward on the same edges: from g_radial, from g_unit, from
    both; the radial rows are bitwise those of the equivariant entry."""
    c = k1_ref.case(2, r_max, nb, p, "random")
    o = _ops()
    pos, ei = _graph(c.vec)
    _, g_rad, g_unit = (_d(t) for t in c.cots)
    rad, unit = o.edge_featurize_gvp(pos, ei, *c.consts)
    got = dict(rad=rad, unit=unit)
    got["gv_rad"] = o.edge_featurize_gvp_bwd(pos, ei, *c.consts, g_rad, None)
    got["gv_unit"] = o.edge_featurize_gvp_bwd(pos, ei, *c.consts, None, g_unit)
    got["gv_both"] = o.edge_featurize_gvp_bwd(pos, ei, *c.consts, g_rad, g_unit)
    torch.cuda.synchronize()
    _zero_length_rows(c, got)
    _past_cutoff_rows(c, got)
    _hold(f"gvp nb={nb}", c, got, ("rad", "unit", "gv_rad", "gv_unit"))
    _joint(c, got, "gv_unit", "gv_rad", "gv_both")
    eq = _run(c, pos_ei=(pos, ei))
    assert _same_bits(eq["rad"], rad) and _same_bits(eq["gv_rad"], got["gv_rad"])
    for rows in (c.cls["cut_at"], c.cls["cut_out"]):
        assert _same_bits(got["gv_both"][rows], got["gv_unit"][rows])


# --------------------------------------------------------------------------------- shifted path
def test_shifted_entry_is_bitwise_the_isolated_edge():
    """pos = 0 everywhere and shift = vec: the _ex entry's prep pass writes (0 - 0) + shift, so it
    gives the isolated-edge result bit for bit, forward and backward, at lmax = 5 (NaN rows of the
    zero-length edges included).  The one thing the prep pass does not carry is the sign of a zero
    component ((0 - 0) + -0.0 is +0.0, and the edge set's negative axis directions hold -0.0):
    bitwise on the vectors with their zeros made +0.0, equal values (0.0 == -0.0) on the raw
    ones."""
    c = k1_ref.case(5, 2.0, 8, 5, "random")
    assert bool(((_bits(c.vec) == -2 ** 31).any()))          # the raw set does hold -0.0
    for vec, same in ((c.vec + 0.0, _same_bits), (c.vec, lambda a, b: torch.equal(
            torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)))):
        pos, ei = _graph(vec, self_loop=False)
        plain = _run(c, vec=vec, pos_ei=(pos, ei))
        shifted = _run(c, vec=vec, shift=vec.to(DEV), pos_ei=(torch.zeros_like(pos), ei))
        for k in plain:
            diff = (_bits(plain[k]) != _bits(shifted[k])).any(dim=-1)
            assert same(plain[k], shifted[k]), (k, int(diff.sum()), diff.nonzero()[:8].tolist())
        _zero_length_rows(c, shifted)


# ---------------------------------------------------------------------------------- grid-stride
def test_second_grid_stride_trip():
    """grid_for_edges caps the grid at 16 blocks per CU: E = cap + 257 edges cycling through a
    4096-vector table take a second trip of the loop.  Every output row, forward and backward,
    is bitwise the row of the same vector from a 4096-edge launch."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = 16 * cus * 256
    T, E = 4096, cap + 257
    assert E * 8 * 4 <= 64 << 20, "outputs stay small"
    c = k1_ref.case(1, 2.0, 1, 5, "random")
    g = torch.Generator().manual_seed(7)
    table = torch.cat([c.vec, torch.randn(T - c.vec.shape[0], 3, generator=g)])
    table = table[torch.randperm(T, generator=g)]
    g_sh, g_rad = torch.randn(T, 4, generator=g).to(DEV), torch.randn(T, 1, generator=g).to(DEV)
    pos, ei = k1_ref.isolated_graph(table)
    pos, ei = pos.to(DEV), ei.to(DEV)
    assert pos.shape[0] == 2 * T
    o = _ops()

    def run(ei_, gs, gr):
        sh, rad = o.edge_featurize(pos, ei_, *c.consts, 1, None)
        return sh, rad, o.edge_featurize_bwd(pos, ei_, *c.consts, gs, gr, 1, None)
    small = run(ei, g_sh, g_rad)
    idx = torch.arange(E, device=DEV) % T
    big = run(ei[:, idx].contiguous(), g_sh[idx], g_rad[idx])
    torch.cuda.synchronize()
    for name, s, b in zip(("sh", "rad", "g_vec"), small, big):
        assert b.shape[0] == E
        same = (_bits(b) == _bits(s)[idx]).all(dim=-1)
        assert bool(same[cap:].all()), (name, "rows of the second trip")
        assert bool(same[-1]), (name, "last row")
        assert bool(same.all()), (name, int((~same).sum()))


# -------------------------------------------------------------------------------------- scatter
def test_scatter_to_pos_vs_fp64():
    """EdgeFeaturizeFn's dpos at lmax = 5 on a 200-node random graph with a node of degree 0, a
    duplicated edge and an edge in both directions: equal to the fp64 scatter of the fp64 per-edge
    g_vec (on the fp32 edge vectors the kernel forms), per node within the sum of the incident
    edges' bounds."""
    from gmp_amd import equivariant as eq
    lmax, N = 5, 200
    blk = k1_ref.radial_block(2.0, 8, 5)
    consts = k1_ref.consts(blk)
    g = torch.Generator().manual_seed(11)
    pos = 1.2 * torch.randn(N, 3, generator=g)
    a = torch.randint(0, N - 1, (1500,), generator=g)
    b = (a + torch.randint(1, N - 1, (1500,), generator=g)) % (N - 1)   # node N - 1: degree 0
    ei = torch.stack([torch.cat([a, a[:1], b[1:2]]), torch.cat([b, b[:1], a[1:2]])])
    E = ei.shape[1]
    assert not bool((ei == N - 1).any()) and not bool((ei[0] == ei[1]).any())
    assert bool((ei[:, 0] == ei[:, E - 2]).all()) and bool((ei[:, 1] == ei[:, E - 1].flip(0)).all())
    vec = pos[ei[0]] - pos[ei[1]]                  # fp32, as the kernel subtracts
    r = vec.double().norm(dim=-1)
    assert int((r < 2.0).sum()) > 100 and int((r > 2.0).sum()) > 100
    g_sh, g_rad = torch.randn(E, 36, generator=g), torch.randn(E, 8, generator=g)
    cots = (g_sh, g_rad, None)
    ref = k1_ref.evaluate(vec, blk, lmax, torch.float64, *cots)
    f32 = k1_ref.evaluate(vec, blk, lmax, torch.float32, *cots)
    u_ref = k1_ref.compare(f32, vec, blk, lmax, cots, ref)
    sc = k1_ref.scales(vec, blk, lmax, *cots)
    # past the cutoff the radial part is exactly zero on both sides (test_cutoff_edges), so it
    # adds nothing to the bound; no edge of this graph is within 1e-5 of r_max
    assert float((r - 2.0).abs().min()) > 1e-5
    assert not bool(ref["gv_rad"][r > 2.0].any())
    bound_e = k1_ref.U24 * (k1_ref.kernel_bound(u_ref["gv_sh"]) * sc["gv_sh"]
                            + k1_ref.kernel_bound(u_ref["gv_rad"]) * sc["gv_rad"] * (r < 2.0))
    gv = ref["gv_sh"] + ref["gv_rad"]
    want = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, ei[0], gv).index_add_(0, ei[1], -gv)
    bound_n = torch.zeros(N, dtype=torch.float64).index_add_(0, ei[0], bound_e)
    bound_n.index_add_(0, ei[1], bound_e)

    pos_d = pos.to(DEV).requires_grad_(True)
    ei_d = ei.to(DEV)
    sh, rad = eq.EdgeFeaturizeFn.apply(pos_d, ei_d, consts, eq.tp_graph(ei_d, N), lmax)
    ((sh * g_sh.to(DEV)).sum() + (rad * g_rad.to(DEV)).sum()).backward()
    dpos = pos_d.grad.cpu().double()
    err = (dpos - want).norm(dim=-1)
    ratio = err[:N - 1] / bound_n[:N - 1]
    print(f"K1 scatter: U_ref gv_sh {u_ref['gv_sh']:.2f} gv_rad {u_ref['gv_rad']:.2f}; worst node "
          f"error / bound {float(ratio.max()):.4f}, median {float(ratio.median()):.4f}")
    assert _is_zero(pos_d.grad[N - 1]) and float(bound_n[N - 1]) == 0.0
    assert bool(torch.isfinite(dpos).all()) and float(ratio.max()) <= 1.0
