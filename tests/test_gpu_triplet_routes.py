"""The routes of K18 / K18d (gmp_sphbasis.hip) and K19 / K19d (gmp_tripletmp.hip) that only large
inputs take, each at the smallest size that selects it, against the fp64 helpers
tests/spherenet_ref.py and tests/dimenet_ref.py.

The other triplet modules run graphs of 24 to 40 points (T of a few thousand), where every block
of triplet_proj_wgrad owns one tile and every wave of interact_bwd / interact1_bwd one edge.  Here
a synthetic triplet list (no 3-D graph: the ops take arbitrary geometry) of E = 8,257 edges and
T ~ 37,000 triplets crosses
  * ceil(T / 64) > 512: a block of triplet_proj_wgrad<true> sums several tiles into one partial
    row, trailing blocks own no tile and write a zero row;
  * E > 8,192: a wave of interact_bwd<8>, interact_bwd<16>, interact1_bwd<8>, interact1_bwd<16>
    walks several edges with its accumulators kept, trailing waves own no edge;
and a second list of T = 4096 * 64 + 65 crosses the same cap of triplet_proj_wgrad<false>.
Every test derives its route from the library's own *_partial_rows numbers and asserts it before
the launch, so a changed cap fails here instead of silently leaving the route uncovered
(tests/test_triplet_routes_host.py pins the same arithmetic without a GPU).

Also here: K19 at I > 64 and ba, bt > 8; the largest bases whose geometry gradient fits the LDS
((8, 6) and (9, 4): n k + n^2 <= 118) and the first refused ones ((9, 5); K19 at I (ba + bt) >
3072), which must raise and leave the leaves without gradients; the per-edge basis gradients at
small and boundary arguments.

Bound: 1e-5 of the fp64 array's own scale, no allowance (_check_scale of the other two modules).

Not reachable in a test of a few seconds, and not covered: tile_grid's cap of 2^20 tiles (67 M
triplets) and the INT32_MAX grid checks of the launchers.  Out-of-range indices and periodic
images are out of scope.
"""
import math

import pytest
import torch

import dimenet_ref as dref
import spherenet_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUTOFF = 5.0
TILE = 64  # triplets per tile of K18 (kTile) and per idx_kj batch of K19 / K19d (kWave)


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _check_scale(name, got, want):
    """1e-5 of the fp64 value's own scale; an identically zero reference must come out zero."""
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    err, bound = _maxabs(got.detach().cpu().double() - want), 1e-5 * _maxabs(want)
    print(f"{name}: err {err:.3e} bound {bound:.3e} err/bound {err / bound if bound else 0.0:.3f}")
    assert err <= bound, (name, err, bound)


def _check_all(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        _check_scale(name, got[name], want[name])


def _ceil_div(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------- routes
def _proj_route(family, T):
    """(partial rows = blocks of triplet_proj_wgrad, tiles per block, trailing blocks without a
    tile) for T triplets, from the library's own row count."""
    from gmp_amd import _lib
    rows = getattr(_lib.load(), f"gmp_{family}_triplet_proj_bwd_partial_rows")(T)
    tiles = _ceil_div(T, TILE)
    tpb = _ceil_div(tiles, rows)
    return rows, tpb, rows - _ceil_div(tiles, tpb)


def _interact_route(name, E):
    """(partial rows = waves of the gradient kernel, edges per wave, trailing waves without an
    edge) for E edges; name is triplet_interact (K19) or triplet_interact1 (K19d)."""
    from gmp_amd import _lib
    rows = getattr(_lib.load(), f"gmp_{name}_bwd_partial_rows")(E)
    epw = _ceil_div(E, rows)
    return rows, epw, rows - _ceil_div(E, epw)


# ----------------------------------------------------------------------------------- the list
_CACHE = {}


def _triplet_list():
    """A seeded synthetic triplet list on the host: counts (E), offs, idx_ji, idx_kj, dist (E),
    angle (T), torsion (T), with the properties _assert_list checks."""
    if "list" in _CACHE:
        return _CACHE["list"]
    E = 8257
    gen = torch.Generator().manual_seed(1907)
    counts = torch.randint(0, 10, (E,), generator=gen)
    counts[0] = 0       # the first wave's first edge
    counts[E - 1] = 0   # the last edge
    counts[1001], counts[1002], counts[5000] = 64, 65, 131
    if int(counts.sum()) % TILE == 0:
        counts[7] += 1
    T = int(counts.sum())
    idx_ji = torch.repeat_interleave(torch.arange(E), counts)
    offs = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    idx_kj = torch.randint(0, E, (T,), generator=gen)
    hub, never = 4321, torch.tensor([0, 77, E - 1])
    idx_kj[torch.isin(idx_kj, never)] = hub
    idx_kj[torch.randperm(T, generator=gen)[:200]] = hub
    dist = 1.0 + 3.9 * torch.rand(E, generator=gen)
    angle = math.pi * torch.rand(T, generator=gen)
    torsion = 2.0 * math.pi * (1.0 - torch.rand(T, generator=gen))
    special = [(th, ph) for th in (0.0, math.pi / 2, math.pi) for ph in (0.0, math.pi, 2 * math.pi)]
    for t in range(12):
        angle[t], torsion[t] = special[t % 9]
    _CACHE["list"] = dict(E=E, T=T, counts=counts, offs=offs, idx_ji=idx_ji, idx_kj=idx_kj,
                          dist=dist, angle=angle, torsion=torsion, special=special)
    return _CACHE["list"]


def _assert_list(lst, epw):
    E, T, counts, kj = lst["E"], lst["T"], lst["counts"], lst["idx_kj"]
    assert counts[0] == 0 and counts[E - 1] == 0 and int((counts == 0).sum()) > 2
    assert int((counts == 64).sum()) >= 1 and int((counts == 65).sum()) >= 1
    assert int(counts.max()) >= 130
    as_kj = torch.bincount(kj, minlength=E)
    assert int(as_kj.max()) >= 200 and int(as_kj.min()) == 0
    f32 = torch.float32
    for t in range(12):
        th, ph = lst["special"][t % 9]
        assert lst["angle"][t] == torch.tensor(th, dtype=f32)
        assert lst["torsion"][t] == torch.tensor(ph, dtype=f32)
    assert {lst["special"][t % 9] for t in range(12)} == set(lst["special"])
    assert T % TILE != 0 and E % epw != 0
    assert int(kj.min()) >= 0 and int(kj.max()) < E and kj.numel() == T
    assert int(lst["offs"][-1]) == T and lst["offs"].numel() == E + 1
    assert torch.equal(lst["idx_ji"], torch.repeat_interleave(torch.arange(E), counts))
    assert lst["dist"].dtype == f32 and lst["angle"].dtype == f32 and lst["torsion"].dtype == f32
    assert float(lst["dist"].min()) >= 1.0 and float(lst["dist"].max()) <= 4.9
    assert float(lst["angle"].min()) >= 0.0 and float(lst["angle"].max()) <= math.pi + 1e-6
    assert float(lst["torsion"].min()) >= 0.0 and float(lst["torsion"].max()) <= 2 * math.pi + 1e-6


def _head(lst, T):
    """The first T triplets of the list, all its edges (the per-triplet kernels only)."""
    out = dict(lst, T=T)
    for key in ("idx_ji", "idx_kj", "angle", "torsion"):
        out[key] = lst[key][:T].clone()
    del out["counts"], out["offs"]
    return out


def _first_edges(lst, E):
    """The first E edges of the list with their triplets, idx_kj folded into [0, E)."""
    T = int(lst["offs"][E])
    return dict(E=E, T=T, counts=lst["counts"][:E].clone(), offs=lst["offs"][:E + 1].clone(),
                idx_ji=lst["idx_ji"][:T].clone(), idx_kj=lst["idx_kj"][:T] % E)


def _tables(n, k):
    from gmp_amd.spherenet import basis_tables
    zeros, norm, pref = basis_tables(n, k)
    return (torch.from_numpy(zeros).to(DEV), torch.from_numpy(norm).to(DEV),
            torch.from_numpy(pref).float().to(DEV))


def _grad(t):
    return t.grad if t.grad is not None else torch.zeros_like(t)


# ----------------------------------------------------------------------------------- SphereNet
def _sphere_inputs(lst, n, k, I, ba, bt, L, interact):
    """fp64 weights and cotangents (values exactly representable in fp32).  With `interact` the
    loss is that of test_gpu_spherenet.test_fused_vs_materialised (m, S[0], P[0], rbf), without
    it every layer's S and P carries a cotangent."""
    E, T = lst["E"], lst["T"]
    gen = torch.Generator().manual_seed(7)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=gen, dtype=torch.float64) * sc).float().double()

    nk, nnk = n * k, n * n * k
    w = {"freq": (torch.arange(1, k + 1, dtype=torch.float64) * torch.pi).float().double()}
    if interact:
        w.update(xd=rnd(E, I), Wa=rnd(I, ba, sc=ba ** -0.5), Wt=rnd(I, bt, sc=bt ** -0.5))
    for l in range(L):
        w[f"W1_{l}"] = rnd(ba, nk, sc=nk ** -0.5)
        w[f"W2_{l}"] = rnd(bt, nnk, sc=nnk ** -0.5)
    cot = {}
    for l in ((0,) if interact else range(L)):
        cot[f"S[{l}]"], cot[f"P[{l}]"] = rnd(T, ba), rnd(T, bt)
    if interact:
        cot["m"] = rnd(E, I)
    return w, cot


def _sphere_gpu(lst, w, cot, n, k, L, interact):
    from gmp_amd import ops
    zt, nt, pt = _tables(n, k)
    wg = {key: v.float().to(DEV).requires_grad_(True) for key, v in w.items()}
    geo = {key: lst[key].to(DEV).requires_grad_(True) for key in ("dist", "angle", "torsion")}
    idx_kj = lst["idx_kj"].to(DEV)
    rbf, jb = ops.SphEdgeBasisFn.apply(geo["dist"], wg["freq"], zt, nt, CUTOFF, 5)
    weights = [wg[f"W1_{l}"] for l in range(L)] + [wg[f"W2_{l}"] for l in range(L)]
    SP = ops.SphTripletProjFn.apply(jb, geo["angle"], geo["torsion"], idx_kj, pt, n, k, L, *weights)
    out = {"rbf": rbf, "jb": jb}
    for l in range(L):
        out[f"S[{l}]"], out[f"P[{l}]"] = SP[l], SP[L + l]
    if interact:
        out["m"] = ops.TripletInteractFn.apply(wg["xd"], SP[1], SP[L + 1], wg["Wa"], wg["Wt"],
                                               idx_kj, lst["idx_ji"].to(DEV), lst["offs"].to(DEV))
    loss = rbf.sum()
    for key, c in cot.items():
        loss = loss + (out[key] * c.float().to(DEV)).sum()
    loss.backward()
    for key, v in list(wg.items()) + list(geo.items()):
        out["grad " + key] = _grad(v)
    return {key: v.detach().cpu() for key, v in out.items()}


def _sphere_ref(lst, w, cot, n, k, L, interact):
    r = {key: v.clone().requires_grad_(True) for key, v in w.items()}
    geo = {key: lst[key].double().requires_grad_(True) for key in ("dist", "angle", "torsion")}
    kj = lst["idx_kj"]
    rbf, jb = sref.edge_basis(geo["dist"], r["freq"], n, k, CUTOFF)
    a, t = sref.triplet_embeddings(jb, geo["angle"], geo["torsion"], kj, n, k)
    out = {"rbf": rbf, "jb": jb}
    for l in range(L):
        out[f"S[{l}]"], out[f"P[{l}]"] = a @ r[f"W1_{l}"].t(), t @ r[f"W2_{l}"].t()
    if interact:
        out["m"] = sref.interact(r["xd"], out["S[1]"], out["P[1]"], r["Wa"], r["Wt"], kj,
                                 lst["idx_ji"], lst["E"])
    loss = rbf.sum()
    for key, c in cot.items():
        loss = loss + (out[key] * c).sum()
    loss.backward()
    for key, v in list(r.items()) + list(geo.items()):
        out["grad " + key] = _grad(v)
    return {key: v.detach() for key, v in out.items()}


FUSED = dict(n=7, k=6, I=64, ba=8, bt=8, L=2)


def _sphere_fused_case():
    """Inputs, routes and the fp64 reference of the fused SphereNet chain, once per session."""
    if "sphere" not in _CACHE:
        lst, s = _triplet_list(), FUSED
        w, cot = _sphere_inputs(lst, s["n"], s["k"], s["I"], s["ba"], s["bt"], s["L"], True)
        _CACHE["sphere"] = (lst, w, cot, _sphere_ref(lst, w, cot, s["n"], s["k"], s["L"], True))
    return _CACHE["sphere"]


def _assert_sphere_routes(lst):
    E, T = lst["E"], lst["T"]
    rows, tpb, idle = _proj_route("sph", T)
    wrows, epw, widle = _interact_route("triplet_interact", E)
    print(f"E {E} T {T}; triplet_proj_wgrad<true>: rows {rows} tiles_per_block {tpb} idle blocks "
          f"{idle}; interact_bwd: rows {wrows} epw {epw} idle waves {widle}")
    _assert_list(lst, epw)
    assert T >= 32769 and tpb >= 2 and idle >= 1
    assert epw >= 2 and widle >= 1


def test_spherenet_fused_multi_tile_multi_edge():
    """SphEdgeBasisFn -> SphTripletProjFn -> TripletInteractFn with tiles_per_block >= 2 in the
    weight gradients of K18 and epw >= 2 in the gradients of K19."""
    lst, w, cot, want = _sphere_fused_case()
    _assert_sphere_routes(lst)
    s = FUSED
    assert max(s["ba"], s["bt"]) <= 8 and s["I"] <= 64  # interact_bwd<8>, one channel per lane
    _check_all(_sphere_gpu(lst, w, cot, s["n"], s["k"], s["L"], True), want)


def test_spherenet_fused_deterministic():
    """Partial rows are summed in a fixed order: two runs of the case above agree bit for bit."""
    lst, w, cot, _ = _sphere_fused_case()
    _assert_sphere_routes(lst)
    s = FUSED
    one = _sphere_gpu(lst, w, cot, s["n"], s["k"], s["L"], True)
    two = _sphere_gpu(lst, w, cot, s["n"], s["k"], s["L"], True)
    assert sorted(one) == sorted(two)
    differ = [key for key in one if not torch.equal(one[key], two[key])]
    assert not differ, differ


# ----------------------------------------------------------------------------------- K19 alone
@pytest.mark.parametrize("I,ba,bt", [(80, 16, 16), (80, 16, 3), (80, 3, 16), (80, 8, 8)])
def test_k19_wide(I, ba, bt):
    """K19 alone on the list, S and P random inputs: I > 64 (a lane serves two channels, gm0 only
    for the first) and, with ba or bt above 8, interact_bwd<16>; epw >= 2."""
    from gmp_amd import ops
    lst = _triplet_list()
    E, T = lst["E"], lst["T"]
    rows, epw, idle = _interact_route("triplet_interact", E)
    kB = 8 if max(ba, bt) <= 8 else 16
    print(f"E {E} T {T} I {I} ba {ba} bt {bt}: interact_bwd<{kB}> rows {rows} epw {epw} idle "
          f"waves {idle}")
    _assert_list(lst, epw)
    assert epw >= 2 and idle >= 1 and I > 64
    assert I * (ba + bt) <= 3072  # the backward's LDS cap
    gen = torch.Generator().manual_seed(13)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=gen, dtype=torch.float64) * sc).float().double()

    w = {"xd": rnd(E, I), "S": rnd(T, ba), "P": rnd(T, bt), "Wa": rnd(I, ba, sc=ba ** -0.5),
         "Wt": rnd(I, bt, sc=bt ** -0.5)}
    cm = rnd(E, I)
    wg = {key: v.float().to(DEV).requires_grad_(True) for key, v in w.items()}
    m = ops.TripletInteractFn.apply(wg["xd"], wg["S"], wg["P"], wg["Wa"], wg["Wt"],
                                    lst["idx_kj"].to(DEV), lst["idx_ji"].to(DEV),
                                    lst["offs"].to(DEV))
    (m * cm.float().to(DEV)).sum().backward()
    r = {key: v.clone().requires_grad_(True) for key, v in w.items()}
    rm = sref.interact(r["xd"], r["S"], r["P"], r["Wa"], r["Wt"], lst["idx_kj"], lst["idx_ji"], E)
    (rm * cm).sum().backward()
    _check_scale("m", m, rm.detach())
    for key in w:
        _check_scale("grad " + key, _grad(wg[key]), r[key].grad)


# ----------------------------------------------------------------------------------- DimeNet++
@pytest.mark.parametrize("b,I", [(8, 64), (16, 80)])
def test_dimenet_fused_multi_edge(b, I):
    """DimeEdgeBasisFn -> DimeTripletProjFn -> TripletInteract1Fn on the list without its torsion:
    interact1_bwd<8> / <16> with epw >= 2, and with I = 80 its second walk over the edges that
    adds to gS."""
    from test_gpu_dimenet import _fused_case
    lst = _triplet_list()
    E, T = lst["E"], lst["T"]
    prows, tpb, pidle = _proj_route("dime", T)
    rows, epw, idle = _interact_route("triplet_interact1", E)
    print(f"E {E} T {T} I {I} b {b}: triplet_proj_wgrad<false> rows {prows} tiles_per_block "
          f"{tpb}; interact1_bwd<{8 if b <= 8 else 16}> rows {rows} epw {epw} idle waves {idle}")
    _assert_list(lst, epw)
    assert epw >= 2 and idle >= 1
    geometry = tuple(lst[key].to(DEV) for key in ("dist", "angle", "idx_kj", "idx_ji", "offs"))
    _fused_case(geometry, 7, 6, I, b, cutoff=CUTOFF)


def test_dimenet_wgrad_cap():
    """K18d alone (edge basis and projections) past the 4096-block cap of
    triplet_proj_wgrad<false>: T = 4096 * 64 + 65 at (n, k) = (3, 2), so that the fp64 reference
    stays at a few MB per array."""
    from gmp_amd import ops
    n, k, b, L, E, T = 3, 2, 8, 2, 500, 4096 * TILE + 65
    rows, tpb, idle = _proj_route("dime", T)
    print(f"E {E} T {T}: triplet_proj_wgrad<false> rows {rows} tiles_per_block {tpb} idle "
          f"blocks {idle}")
    assert T >= 262145 and T % TILE != 0 and tpb >= 2 and idle >= 1
    gen = torch.Generator().manual_seed(23)
    idx_kj = torch.randint(0, E, (T,), generator=gen)
    dist = 1.0 + 3.9 * torch.rand(E, generator=gen)
    angle = math.pi * torch.rand(T, generator=gen)
    angle[:3] = torch.tensor([0.0, math.pi / 2, math.pi])
    nk = n * k
    w = {"freq": (torch.arange(1, k + 1, dtype=torch.float64) * torch.pi).float().double()}
    for l in range(L):
        w[f"W1_{l}"] = (torch.randn(b, nk, generator=gen, dtype=torch.float64)
                        * nk ** -0.5).float().double()
    cot = [torch.randn(T, b, generator=gen) for _ in range(L)]

    zt, nt, pt = _tables(n, k)
    wg = {key: v.float().to(DEV).requires_grad_(True) for key, v in w.items()}
    geo = {"dist": dist.to(DEV).requires_grad_(True), "angle": angle.to(DEV).requires_grad_(True)}
    rbf, sbe = ops.DimeEdgeBasisFn.apply(geo["dist"], wg["freq"], zt, nt, CUTOFF, 5)
    S = ops.DimeTripletProjFn.apply(sbe, geo["angle"], idx_kj.to(DEV), pt, n, k, L,
                                    *[wg[f"W1_{l}"] for l in range(L)])
    loss = rbf.sum()
    for l in range(L):
        loss = loss + (S[l] * cot[l].to(DEV)).sum()
    loss.backward()

    r = {key: v.clone().requires_grad_(True) for key, v in w.items()}
    rgeo = {"dist": dist.double().requires_grad_(True), "angle": angle.double().requires_grad_(True)}
    rrbf, rsbe = dref.edge_basis(rgeo["dist"], r["freq"], n, k, CUTOFF)
    rsbf = dref.triplet_embedding(rsbe, rgeo["angle"], idx_kj, n, k)
    rS = [rsbf @ r[f"W1_{l}"].t() for l in range(L)]
    rloss = rrbf.sum()
    for l in range(L):
        rloss = rloss + (rS[l] * cot[l].double()).sum()
    rloss.backward()
    _check_scale("rbf", rbf, rrbf.detach())
    _check_scale("sbe", sbe, rsbe.detach())
    for l in range(L):
        _check_scale(f"S[{l}]", S[l], rS[l].detach())
    for key in w:
        _check_scale("grad " + key, _grad(wg[key]), _grad(r[key]))
    for key in geo:
        _check_scale("grad " + key, _grad(geo[key]), _grad(rgeo[key]))


# ----------------------------------------------------------------------------------- basis sizes
@pytest.mark.parametrize("n,k", [(8, 6), (9, 4)])
def test_largest_bases(n, k):
    """The largest bases whose geometry gradient fits the LDS (2 tile_lds <= 60 KiB: n k + n^2 <=
    118), on the first 333 triplets of the list (the special angles among them): the fp32 Legendre
    and C_m / S_m recurrences above l = 6."""
    assert n * k + n * n <= 118 < (n + 1) * k + (n + 1) ** 2
    lst = _head(_triplet_list(), 333)
    ba = bt = 8
    L = 2
    print(f"(n, k) = ({n}, {k}): E {lst['E']} T {lst['T']}, geometry gradient LDS "
          f"{2 * (n * k + n * n) * 65 * 4} B")
    w, cot = _sphere_inputs(lst, n, k, 0, ba, bt, L, False)
    want = _sphere_ref(lst, w, cot, n, k, L, False)
    _check_all(_sphere_gpu(lst, w, cot, n, k, L, False), want)


def test_first_refused_basis():
    """(n, k) = (9, 5), n k + n^2 = 126: the forward is accepted (and right), the geometry
    gradient is GMP_ERR_UNSUPPORTED: backward() raises and writes no gradient."""
    from gmp_amd import ops
    n, k, ba, bt, L = 9, 5, 8, 8, 2
    assert n * k + n * n > 118
    lst = _head(_triplet_list(), 333)
    E, T = lst["E"], lst["T"]
    print(f"(n, k) = ({n}, {k}): E {E} T {T}")
    w, cot = _sphere_inputs(lst, n, k, 0, ba, bt, L, False)
    _, _, pt = _tables(n, k)
    gen = torch.Generator().manual_seed(29)
    jb64 = torch.randn(E, n * k, generator=gen, dtype=torch.float64).float().double()
    leaves = {key: w[key].float().to(DEV).requires_grad_(True) for key in w if key != "freq"}
    leaves["jb"] = jb64.float().to(DEV).requires_grad_(True)
    for key in ("angle", "torsion"):
        leaves[key] = lst[key].to(DEV).requires_grad_(True)
    weights = [leaves[f"W1_{l}"] for l in range(L)] + [leaves[f"W2_{l}"] for l in range(L)]
    SP = ops.SphTripletProjFn.apply(leaves["jb"], leaves["angle"], leaves["torsion"],
                                    lst["idx_kj"].to(DEV), pt, n, k, L, *weights)
    a, t = sref.triplet_embeddings(jb64, lst["angle"].double(), lst["torsion"].double(),
                                   lst["idx_kj"], n, k)
    for l in range(L):
        _check_scale(f"S[{l}]", SP[l], a @ w[f"W1_{l}"].t())
        _check_scale(f"P[{l}]", SP[L + l], t @ w[f"W2_{l}"].t())
    loss = sum((SP[l] * cot[f"S[{l}]"].float().to(DEV)).sum()
               + (SP[L + l] * cot[f"P[{l}]"].float().to(DEV)).sum() for l in range(L))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        loss.backward()
    torch.cuda.synchronize()
    assert [key for key, v in leaves.items() if v.grad is not None] == []


def test_k19_first_refused_width():
    """K19 at I = 128, ba = bt = 16: I (ba + bt) = 4096 floats of weights fit the forward's LDS
    (and the forward is right), five times that does not fit the backward's: backward() raises and
    writes no gradient."""
    from gmp_amd import ops
    I, ba, bt = 128, 16, 16
    assert I * (ba + bt) > 3072 and I * (ba + bt) * 4 <= 60 * 1024
    lst = _first_edges(_triplet_list(), 300)
    E, T = lst["E"], lst["T"]
    print(f"E {E} T {T} I {I} ba {ba} bt {bt}")
    assert T > 0 and int(lst["counts"].max()) > 0
    gen = torch.Generator().manual_seed(31)

    def rnd(*sh, sc=1.0):
        return (torch.randn(*sh, generator=gen, dtype=torch.float64) * sc).float().double()

    w = {"xd": rnd(E, I), "S": rnd(T, ba), "P": rnd(T, bt), "Wa": rnd(I, ba, sc=ba ** -0.5),
         "Wt": rnd(I, bt, sc=bt ** -0.5)}
    leaves = {key: v.float().to(DEV).requires_grad_(True) for key, v in w.items()}
    m = ops.TripletInteractFn.apply(leaves["xd"], leaves["S"], leaves["P"], leaves["Wa"],
                                    leaves["Wt"], lst["idx_kj"].to(DEV), lst["idx_ji"].to(DEV),
                                    lst["offs"].to(DEV))
    _check_scale("m", m, sref.interact(w["xd"], w["S"], w["P"], w["Wa"], w["Wt"], lst["idx_kj"],
                                       lst["idx_ji"], E))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        m.sum().backward()
    torch.cuda.synchronize()
    assert [key for key, v in leaves.items() if v.grad is not None] == []


# ----------------------------------------------------------------------------------- per edge
SMALL_X = (0.01, 0.02, 0.05, 0.1, 0.2, 0.999)


def _edge_family(family):
    from gmp_amd import ops
    if family == "sph":
        return ops.SphEdgeBasisFn, sref.edge_basis
    return ops.DimeEdgeBasisFn, dref.edge_basis


def _edge_basis_grads(family, dist, n, k, c_rbf, c_jb):
    """(values and gradients on the GPU, the same from the fp64 helper's autograd) for the loss
    sum(rbf c_rbf) + sum(jb c_jb); dist fp32 on the host, the cotangents fp64."""
    fn, ref_basis = _edge_family(family)
    zt, nt, _ = _tables(n, k)
    freq = (torch.arange(1, k + 1, dtype=torch.float64) * torch.pi).float()
    gd, gf = dist.to(DEV).requires_grad_(True), freq.to(DEV).requires_grad_(True)
    rbf, jb = fn.apply(gd, gf, zt, nt, CUTOFF, 5)
    ((rbf * c_rbf.float().to(DEV)).sum() + (jb * c_jb.float().to(DEV)).sum()).backward()
    got = {"rbf": rbf, "jb": jb, "grad dist": _grad(gd), "grad freq": _grad(gf)}
    rd, rf = dist.double().requires_grad_(True), freq.double().requires_grad_(True)
    rrbf, rjb = ref_basis(rd, rf, n, k, CUTOFF)
    ((rrbf * c_rbf).sum() + (rjb * c_jb).sum()).backward()
    want = {"rbf": rrbf, "jb": rjb, "grad dist": _grad(rd), "grad freq": _grad(rf)}
    return ({key: v.detach().cpu() for key, v in got.items()},
            {key: v.detach() for key, v in want.items()})


@pytest.mark.parametrize("family", ["sph", "dime"])
def test_edge_basis_grad_small_x(family):
    """grad_dist and grad_freq at dist / cutoff down to 0.01 and up to 0.999, through rbf alone and
    through the columns of each order l alone (the orders differ by x^l, so one loss over all
    columns would only see l = 0).  Besides the bound on the array, each edge's grad_dist is within
    1e-5 of its own fp64 value: the per-edge arithmetic is double rounded once to fp32 (6e-8), and
    no sum here cancels by anything near the 1e9 it would take to show in double."""
    n, k = 7, 6
    dist = (torch.tensor(SMALL_X, dtype=torch.float64) * CUTOFF).float()
    E = dist.numel()
    gen = torch.Generator().manual_seed(37)
    c_rbf = torch.randn(E, k, generator=gen, dtype=torch.float64).float().double()
    c_jb = torch.randn(E, n * k, generator=gen, dtype=torch.float64).float().double()
    print(f"{family}: x = {SMALL_X}")
    for part in ["rbf"] + list(range(n)):
        if part == "rbf":
            a, b = c_rbf, torch.zeros_like(c_jb)
        else:
            a, b = torch.zeros_like(c_rbf), torch.zeros_like(c_jb)
            b[:, part * k:(part + 1) * k] = c_jb[:, part * k:(part + 1) * k]
        got, want = _edge_basis_grads(family, dist, n, k, a, b)
        tag = f"{family} through {'rbf' if part == 'rbf' else f'l = {part}'}: "
        _check_scale(tag + "grad dist", got["grad dist"], want["grad dist"])
        _check_scale(tag + "grad freq", got["grad freq"], want["grad freq"])
        rel = (got["grad dist"].double() - want["grad dist"]).abs() / want["grad dist"].abs()
        print(tag + "grad dist per edge, relative:", [f"{v:.1e}" for v in rel.tolist()])
        assert float(want["grad dist"].abs().min()) > 0 and float(rel.max()) <= 1e-5, (tag, rel)


def test_dimenet_exact_cutoff():
    """DimeNet++ at dist == cutoff exactly (exact zeros of value and gradient, PyG's [x < 1]) and
    one fp32 step below it (finite, non-zero, and with the other edges within the bound).  There
    the envelope is 56 (1 - x)^3 = 4.9e-20, below what its four-term form resolves in double
    (3.5e-15): the fp64 helper returns exact zeros for that edge and the kernel, with fused
    multiply-adds, a residue (measured: |rbf| 1.4e-21, |sbe| 3.5e-21).  Non-zero therefore says
    that the edge is live, not that its digits are right; both are zero at the bound's scale."""
    n, k = 7, 6
    dist = torch.tensor([CUTOFF, 0.0, 2.5, 1.0, 4.0, 1.5 * CUTOFF], dtype=torch.float32)
    dist[1] = torch.nextafter(dist[0], torch.tensor(0.0))
    assert float(dist[0]) == CUTOFF and float(dist[1]) == CUTOFF - 2.0 ** -21  # fp32 neighbour
    E = dist.numel()
    gen = torch.Generator().manual_seed(41)
    c_rbf = torch.randn(E, k, generator=gen, dtype=torch.float64).float().double()
    c_jb = torch.randn(E, n * k, generator=gen, dtype=torch.float64).float().double()
    got, want = _edge_basis_grads("dime", dist, n, k, c_rbf, c_jb)
    for e in (0, 5):  # at and beyond the cutoff
        assert _maxabs(got["rbf"][e]) == 0.0 and _maxabs(got["jb"][e]) == 0.0
        assert float(got["grad dist"][e]) == 0.0
    for key in ("rbf", "jb"):
        row = got[key][1]
        print(f"{key} one step below the cutoff: max |value| {_maxabs(row):.3e} "
              f"(fp64 {_maxabs(want[key][1]):.3e})")
        assert bool(torch.isfinite(row).all()) and _maxabs(row) > 0.0
    assert math.isfinite(float(got["grad dist"][1]))
    _check_all(got, want)
