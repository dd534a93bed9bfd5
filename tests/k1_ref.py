"""fp64 reference of K1 (csrc/gmp_featurize.hip: featurize_fwd_kernel, featurize_bwd_kernel), the
edge sets the tests run it on, and the per-entry / per-edge error scales they hold it to.  Pure
torch on the CPU oracle; importable without a GPU.

The reference is the oracle itself in float64 on the fp32 edge vectors and the fp32 module
buffers: oracle.o3.spherical_harmonics, oracle.radial.RadialEmbeddingBlock(...).double(),
nan_to_num(vec / |vec|), and per-edge g_vec by autograd (every edge is its own leaf row, so one
backward gives the per-edge gradients with no scatter in between).

Scales.  Every comparison is |got - ref64| <= K 2^-24 scale, entry by entry (forward) or edge by
edge on the 3-vector's norm (backward); no global maximum anywhere.  With r = |vec|, u = r / r_max,
w_n the Bessel weights, c1 = (p+1)(p+2)/2, c2 = p(p+2), c3 = p(p+1)/2 and
    A(u)  = 1 + c1 u^p + c2 u^(p+1) + c3 u^(p+2)            (the envelope's terms, absolute values)
    A'(u) = (c1 p u^(p-1) + c2 (p+1) u^p + c3 (p+2) u^(p+1)) / r_max
the scales are
    sh[e, l block]   sqrt(2l + 1)                              (|Y_l| on the unit sphere)
    radial[e, n]     prefactor (1/r + w_n) A(u)
    unit[e, k]       1
    g_vec from g_sh      (1/r) sum_{l>=1} sqrt(l(l+1)(2l+1)) |g_l|     (Frobenius norm of grad Y_l)
    g_vec from g_radial  sum_n |g_n| prefactor ((w_n/r + 1/r^2 + w_n^2) A(u) + (1/r + w_n) A'(u))
    g_vec from g_unit    |g_unit| / r
A relative check of the radial block is not possible: near the cutoff the envelope is a
cancellation to (1 - u)^3 and the fp32 oracle itself is off by a large relative factor there.

K is not a constant of this file.  evaluate(..., torch.float32) is the oracle run in float32 on
the same inputs; its own worst error in these units is U_ref, and the kernels are held to
4 max(U_ref, 1) (device sinf / powf of a couple of ulp where the CPU's are nearly correctly
rounded, and another FMA contraction).  REF_CAP is the cap the host test holds U_ref to.
"""
import copy
import functools
import itertools
import math
import types

import torch

from oracle import o3 as oo3
from oracle.radial import RadialEmbeddingBlock

U24 = 2.0 ** -24
REF_CAP = 16.0      # units the fp32 oracle stays under on every edge set below (host test)
KERNEL_FACTOR = 4.0


def radial_block(r_max, nb, p):
    """The oracle's radial block; its fp32 buffers are the constants of kernel and reference."""
    return RadialEmbeddingBlock(r_max, nb, p)


def consts(block):
    """(bessel weights, prefactor, r_max, p) as Python floats of the fp32 buffers: the argument
    list of the torch ops after (pos, edge_index)."""
    b = block.bessel_fn
    return ([float(v) for v in b.bessel_weights], float(b.prefactor), float(block.cutoff_fn.r_max),
            float(block.cutoff_fn.p))


def _f32(x):
    return torch.as_tensor(x, dtype=torch.float64).float()


def _dirs(g, n):
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return torch.nn.functional.normalize(v, dim=-1)


def structured_directions():
    """name -> (k, 3) float64: the 6 axis directions, the 12 face diagonals, the 8 body diagonals
    and directions a hair off an axis ((1e-4, 0, 0.7) and its permutations, both signs of the
    small component).  Not normalised: the radii of edge_set scale them."""
    axis = [s * torch.eye(3, dtype=torch.float64)[k] for k in range(3) for s in (1.0, -1.0)]
    face = []
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for si, sj in itertools.product((1.0, -1.0), repeat=2):
            v = torch.zeros(3, dtype=torch.float64)
            v[i], v[j] = si, sj
            face.append(v / math.sqrt(2.0))
    body = [torch.tensor(s, dtype=torch.float64) / math.sqrt(3.0)
            for s in itertools.product((1.0, -1.0), repeat=3)]
    near = []
    for perm in itertools.permutations((1e-4, 0.0, 0.7)):
        for s in (1.0, -1.0):
            v = torch.tensor(perm, dtype=torch.float64)
            near.append(torch.where(v == 1e-4, s * v, v) / 0.7)
    return dict(axis=torch.stack(axis), face=torch.stack(face), body=torch.stack(body),
                near_axis=torch.stack(near))


def edge_set(r_max, n_random=1024, seed=0):
    """(vec (E, 3) float32, classes: name -> index tensor).  r_max is the fp32 buffer's value.
      log, uniform   random directions, r log-spaced 1e-6 .. just under r_max / uniform in
                     [0, 1.5 r_max]
      axis, face, body, near_axis   structured_directions() at seven radii inside the cutoff
      cut_at    (r_max, 0, 0) and the other five axis directions: r == r_max exactly
      cut_in    nextafter(r_max, 0) on each axis
      cut_out   nextafter(r_max, inf) on each axis, and 2 r_max
      zero      vec = 0 (twice: isolated_graph turns the last one into a true self-loop)
    """
    g = torch.Generator().manual_seed(seed)
    rm = float(_f32(r_max))
    assert rm == r_max, "r_max must be fp32-representable"
    parts, classes, n = [], {}, 0

    def add(name, v):
        nonlocal n
        v = v.float()
        parts.append(v)
        classes[name] = torch.arange(n, n + len(v))
        n += len(v)

    r_log = torch.logspace(-6, math.log10(rm * (1 - 1e-6)), n_random, dtype=torch.float64)
    add("log", _dirs(g, n_random) * r_log[:, None])
    r_uni = torch.rand(n_random, generator=g, dtype=torch.float64) * 1.5 * rm
    add("uniform", _dirs(g, n_random) * r_uni[:, None])
    radii = torch.tensor([1e-5, 1e-3, 0.05, 0.31, 0.5, 0.77, 0.96], dtype=torch.float64) * rm
    for name, d in structured_directions().items():
        add(name, (d[None, :, :] * radii[:, None, None]).reshape(-1, 3))
    eye = torch.cat([torch.eye(3), -torch.eye(3)]).double()
    below = float(torch.nextafter(_f32(rm), _f32(0.0)))
    above = float(torch.nextafter(_f32(rm), _f32(math.inf)))
    add("cut_at", eye * rm)
    add("cut_in", eye * below)
    add("cut_out", torch.cat([eye * above, eye * (2 * rm)]))
    add("zero", torch.zeros(2, 3, dtype=torch.float64))
    return torch.cat(parts), classes


def onehot_edge_set(r_max, lmax, n_random=512, seed=1):
    """(vec, classes, col): every structured direction at three radii, once per SH column (so each
    column of the Jacobian meets each of those directions), then random edges whose column is
    e mod nsh.  col (E,) is the column of edge e's one-hot g_sh."""
    nsh = (lmax + 1) ** 2
    g = torch.Generator().manual_seed(seed)
    radii = torch.tensor([1e-4, 0.4, 0.9], dtype=torch.float64) * r_max
    parts, cols, classes, n = [], [], {}, 0
    for name, d in structured_directions().items():
        v = (d[None, :, :] * radii[:, None, None]).reshape(-1, 3)
        parts.append(v.repeat(nsh, 1))
        cols.append(torch.arange(nsh).repeat_interleave(len(v)))
        classes[name] = torch.arange(n, n + nsh * len(v))
        n += nsh * len(v)
    r = torch.rand(n_random, generator=g, dtype=torch.float64) * 1.2 * r_max + 1e-3
    parts.append(_dirs(g, n_random) * r[:, None])
    cols.append(torch.arange(n_random) % nsh)
    classes["uniform"] = torch.arange(n, n + n_random)
    return torch.cat(parts).float(), classes, torch.cat(cols)


# (lmax, r_max, num_bessel, p) of the GPU cases; the host test runs the fp32 oracle on the same
CASES_LMAX = [(lmax, 2.0, 8, 5) for lmax in range(6)]
CASES_RADIAL = [(2, 3.7, 1, 5), (2, 3.7, 32, 5), (2, 3.7, 8, 6), (2, 3.7, 8, 2)]


@functools.lru_cache(maxsize=None)
def case(lmax, r_max, nb, p, kind):
    """One (parameters, edge set, cotangents) case with its fp64 reference, the fp32 oracle's
    result and U_ref per quantity; computed once and shared (nobody writes to it).  kind: the
    cotangents() kinds on edge_set(), or "onehot_tiled" on onehot_edge_set()."""
    blk = radial_block(r_max, nb, p)
    rm = consts(blk)[2]
    if kind == "onehot_tiled":
        vec, cls, col = onehot_edge_set(rm, lmax)
        cots = cotangents(vec, blk, lmax, "onehot", col=col)
    else:
        vec, cls = edge_set(rm)
        cots = cotangents(vec, blk, lmax, kind)
    ref = evaluate(vec, blk, lmax, torch.float64, *cots)
    f32 = evaluate(vec, blk, lmax, torch.float32, *cots)
    return types.SimpleNamespace(lmax=lmax, blk=blk, consts=consts(blk), vec=vec, cls=cls,
                                 cots=cots, ref=ref, f32=f32,
                                 u_ref=compare(f32, vec, blk, lmax, cots, ref))


def isolated_graph(vec, self_loop_last=False):
    """pos (2E, 3), edge_index (2, E): edge e = (2e, 2e + 1), pos[2e] = vec_e, pos[2e + 1] = 0,
    so pos[a] - pos[b] is vec_e exactly.  self_loop_last: the last edge (whose vec must be 0)
    becomes (2E - 2, 2E - 2) with a non-zero position."""
    E = vec.shape[0]
    pos = torch.zeros(2 * E, 3)
    pos[0::2] = vec
    ei = torch.stack([torch.arange(0, 2 * E, 2), torch.arange(1, 2 * E, 2)])
    if self_loop_last:
        assert not bool(vec[-1].any())
        pos[2 * E - 2] = torch.tensor([0.3, -1.2, 0.7])
        ei[1, E - 1] = 2 * E - 2
    return pos, ei


def sh_of(vec, lmax, dtype=torch.float64):
    return oo3.spherical_harmonics(vec.to(dtype), lmax)


def evaluate(vec, block, lmax, dtype, g_sh=None, g_rad=None, g_unit=None):
    """The oracle in `dtype` on the fp32 vectors: dict of sh (E, (lmax+1)^2), rad (E, nb), unit
    (E, 3) and, for each cotangent given, the per-edge g_vec it alone produces (gv_sh, gv_rad,
    gv_unit; all detached, in `dtype`).  Rows of zero-length edges hold what torch gives there
    (NaN radial rows, NaN gradients); the callers pin those rows separately."""
    blk = copy.deepcopy(block).to(dtype)
    v = vec.detach().to(dtype).clone().requires_grad_(True)
    sh = oo3.spherical_harmonics(v, lmax)
    r = torch.linalg.norm(v, dim=-1, keepdim=True)
    rad = blk(r)
    unit = torch.nan_to_num(v / r)
    out = dict(sh=sh.detach(), rad=rad.detach(), unit=unit.detach())
    for name, y, g in (("gv_sh", sh, g_sh), ("gv_rad", rad, g_rad), ("gv_unit", unit, g_unit)):
        if g is None:
            continue
        assert g.dtype == torch.float32 and g.shape == y.shape, (name, g.shape, y.shape)
        if y.numel() == 0 or not y.requires_grad:
            out[name] = torch.zeros_like(v).detach()
            continue
        gv, = torch.autograd.grad((y * g.to(dtype)).sum(), v, retain_graph=True, allow_unused=True)
        out[name] = torch.zeros_like(v).detach() if gv is None else gv.detach()
    return out


def _envelope_abs(u, p, r_max):
    c1, c2, c3 = (p + 1) * (p + 2) / 2, p * (p + 2), p * (p + 1) / 2
    A = 1 + c1 * u ** p + c2 * u ** (p + 1) + c3 * u ** (p + 2)
    dA = (c1 * p * u ** (p - 1) + c2 * (p + 1) * u ** p + c3 * (p + 2) * u ** (p + 1)) / r_max
    return A, dA


def scales(vec, block, lmax, g_sh=None, g_rad=None, g_unit=None):
    """The error scales of the module docstring in float64: sh (nsh,), rad (E, nb), unit 1.0, and
    per edge gv_sh, gv_rad, gv_unit for the cotangents given.  Rows with r = 0 hold inf (never
    compared)."""
    w, pref, r_max, p = consts(block)
    w = torch.tensor(w, dtype=torch.float64)
    r = torch.linalg.norm(vec.double(), dim=-1)
    inv = 1.0 / r
    A, dA = _envelope_abs(r / r_max, p, r_max)
    out = dict(unit=1.0)
    out["sh"] = torch.cat([torch.full((2 * l + 1,), math.sqrt(2 * l + 1), dtype=torch.float64)
                           for l in range(lmax + 1)])
    out["rad"] = pref * (inv[:, None] + w[None, :]) * A[:, None]
    if g_sh is not None:
        s = torch.zeros_like(r)
        for l in range(1, lmax + 1):
            g_l = g_sh[:, l * l:(l + 1) ** 2].double()
            s += math.sqrt(l * (l + 1) * (2 * l + 1)) * g_l.norm(dim=-1)
        out["gv_sh"] = s * inv
    if g_rad is not None:
        wn, ir = w[None, :], inv[:, None]
        J = pref * ((wn * ir + ir ** 2 + wn ** 2) * A[:, None] + (ir + wn) * dA[:, None])
        out["gv_rad"] = (g_rad.double().abs() * J).sum(-1)
    if g_unit is not None:
        out["gv_unit"] = g_unit.double().norm(dim=-1) * inv
    return out


def units(got, ref, scale, vector=False):
    """|got - ref| / (2^-24 scale) per entry, or per row on the row's norm (vector=True; scale
    per row).  scale broadcasts against the result.  A zero scale counts 0 where got == ref and
    inf elsewhere; a non-finite difference counts inf."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = got - ref
    err = err.norm(dim=-1) if vector else err.abs()
    scale = torch.as_tensor(scale, dtype=torch.float64).expand_as(err)
    q = torch.where(scale > 0, err / (U24 * scale.clamp_min(1e-300)),
                    torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return torch.where(torch.isfinite(err), q, torch.full_like(q, math.inf))


def worst(got, ref, scale, rows=None, vector=False):
    """max of units() over the rows given (index tensor; default all); scale is indexed with the
    rows when it is per row (a leading dimension of the edge count)."""
    scale = torch.as_tensor(scale, dtype=torch.float64)
    if rows is not None:
        if scale.dim() > 0 and scale.dim() == (1 if vector else got.dim()):
            scale = scale[rows]
        got, ref = got.detach().cpu()[rows], ref[rows]
    q = units(got, ref, scale, vector)
    return float(q.max()) if q.numel() else 0.0


def kernel_bound(u_ref):
    """4 max(U_ref, 1) units: what the kernels are held to, from the fp32 oracle's own error."""
    return KERNEL_FACTOR * max(u_ref, 1.0)


def cotangents(vec, block, lmax, kind, seed=0, col=None):
    """fp32 cotangents (g_sh (E, nsh), g_rad (E, nb), g_unit (E, 3)).
      random   N(0, 1)
      radial   g_sh = c_e Y(vec_e) (Y in fp64, rounded to fp32; c_e in [0.5, 2]): the true g_vec
               is a cancellation to ~0, left over only if the - u (u . du) projection is missing
      onehot   g_sh[e] = the unit row of column col[e] (default e mod nsh)
    g_rad and g_unit are random in every kind."""
    g = torch.Generator().manual_seed(1000 + seed)
    E, nsh, nb = vec.shape[0], (lmax + 1) ** 2, block.out_dim
    g_rad = torch.randn(E, nb, generator=g)
    g_unit = torch.randn(E, 3, generator=g)
    if kind == "random":
        g_sh = torch.randn(E, nsh, generator=g)
    elif kind == "radial":
        c = 0.5 + 1.5 * torch.rand(E, 1, generator=g, dtype=torch.float64)
        g_sh = (c * sh_of(vec, lmax)).float()
    elif kind == "onehot":
        g_sh = torch.zeros(E, nsh)
        g_sh[torch.arange(E), torch.arange(E) % nsh if col is None else col] = 1.0
    else:
        raise ValueError(kind)
    return g_sh, g_rad, g_unit


def live_rows(vec):
    """Indices of the edges with r > 0 (the ones compared with the fp64 reference)."""
    return torch.nonzero(vec.double().norm(dim=-1) > 0).reshape(-1)


def compare(got, vec, block, lmax, cots, ref=None, rows=None):
    """Worst error in units per quantity of `got` (a dict with any of sh, rad, unit, gv_sh,
    gv_rad, gv_unit) against the fp64 reference, over the rows with r > 0 (or the rows given)."""
    g_sh, g_rad, g_unit = cots
    ref = ref if ref is not None else evaluate(vec, block, lmax, torch.float64, *cots)
    sc = scales(vec, block, lmax, *cots)
    rows = live_rows(vec) if rows is None else rows
    out = {}
    for k in ("sh", "rad", "unit", "gv_sh", "gv_rad", "gv_unit"):
        if k in got and k in ref:
            out[k] = worst(got[k], ref[k], sc[k], rows, vector=k.startswith("gv_"))
    return out
