"""Host-side checks of the K1 reference and its error scales (tests/k1_ref.py; no GPU): the fp32
oracle stays under k1_ref.REF_CAP units on the exact edge sets, parameters and cotangents of
tests/test_gpu_k1_edges.py, so the scales are right and the inputs are ones a correct fp32
evaluation passes; the scales are not loose (one entry moved by 1e-5 of its scale, or one l = 4 / 5
entry with a flipped sign on an axis edge, breaks even the loosest bound a kernel can get,
4 REF_CAP units); the fp64 blocks have |Y_l|^2 = 2l + 1."""
import pytest
import torch

import k1_ref

LOOSEST = k1_ref.kernel_bound(k1_ref.REF_CAP)   # no kernel bound can exceed this many units
QUANTITIES = ("sh", "rad", "unit", "gv_sh", "gv_rad", "gv_unit")


def _case(lmax, r_max, nb, p, kind):
    c = k1_ref.case(lmax, r_max, nb, p, kind)
    return c.blk, c.vec, c.cls, c.cots, c.ref, c.f32


@pytest.mark.parametrize("lmax,r_max,nb,p,kind",
                         [c + ("random",) for c in k1_ref.CASES_LMAX + k1_ref.CASES_RADIAL]
                         + [(5, 2.0, 8, 5, "radial"), (5, 2.0, 8, 5, "onehot"),
                            (5, 2.0, 8, 5, "onehot_tiled"), (2, 3.7, 0, 5, "random")])
def test_fp32_oracle_within_cap(lmax, r_max, nb, p, kind):
    blk, vec, cls, cots, ref, f32 = _case(lmax, r_max, nb, p, kind)
    u = k1_ref.compare(f32, vec, blk, lmax, cots, ref)
    print(f"U_ref lmax={lmax} r_max={r_max} nb={nb} p={p} {kind} (E={len(vec)}):",
          {k: round(v, 2) for k, v in u.items()})
    assert set(u) == set(QUANTITIES)
    assert max(u.values()) <= k1_ref.REF_CAP, u
    # the fp64 reference agrees with the kernel's rule at and past the cutoff: exact zeros
    for name in ("cut_at", "cut_out"):
        if name in cls:
            assert not bool(ref["rad"][cls[name]].any())
            assert not bool(ref["gv_rad"][cls[name]].any())
            if kind == "random" and lmax >= 1:   # the SH part does not stop at the cutoff
                assert bool((ref["gv_sh"][cls[name]].norm(dim=-1) > 0).all())


def test_radial_cotangent_is_a_cancellation():
    """g_sh = c Y: the fp64 g_vec is ~0 (1e-6 of its scale or less) on every edge, so whatever a
    kernel returns there beyond rounding is a missing projection.  Without the - u (u . du) term
    the result keeps u (u . du) / r with u . du = sum_l l g_l . Y_l (Y_l is homogeneous of degree
    l): that fails on every edge."""
    blk, vec, cls, cots, ref, _ = _case(5, 2.0, 8, 5, "radial")
    rows = k1_ref.live_rows(vec)
    sc = k1_ref.scales(vec, blk, 5, *cots)["gv_sh"][rows]
    assert float((ref["gv_sh"][rows].norm(dim=-1) / sc).max()) < 1e-6
    v = vec.double()[rows]
    r = v.norm(dim=-1, keepdim=True)
    udu = sum(l * (cots[0].double()[rows, l * l:(l + 1) ** 2]
                   * ref["sh"][rows, l * l:(l + 1) ** 2]).sum(-1, keepdim=True) for l in range(1, 6))
    unprojected = ref["gv_sh"][rows] + v / r * udu / r
    q = k1_ref.units(unprojected, ref["gv_sh"][rows], sc, vector=True)
    assert float(q.min()) > LOOSEST, float(q.min())


@pytest.mark.parametrize("lmax,r_max,nb,p", [(5, 2.0, 8, 5), (2, 3.7, 32, 5)])
def test_scales_are_not_loose(lmax, r_max, nb, p):
    """One entry of the fp64 result moved by 1e-5 of its scale, on the first, middle and last edge
    of every class: every one of them breaks the loosest bound."""
    blk, vec, cls, cots, ref, _ = _case(lmax, r_max, nb, p, "random")
    sc = k1_ref.scales(vec, blk, lmax, *cots)
    missed = []
    for name, idx in cls.items():
        if name == "zero":
            continue
        for e in {int(idx[0]), int(idx[len(idx) // 2]), int(idx[-1])}:
            for q in QUANTITIES:
                bad = {k: v.clone() for k, v in ref.items()}
                j = (e + 1) % bad[q].shape[1]
                s = sc[q]
                s = float(s) if not torch.is_tensor(s) else float(s[j] if q == "sh" else
                                                                  s[e] if s.dim() == 1 else s[e, j])
                bad[q][e, j] += 1e-5 * s
                w = k1_ref.compare(bad, vec, blk, lmax, cots, ref, rows=torch.tensor([e]))
                if not w[q] > LOOSEST:
                    missed.append((name, e, q, w[q]))
                assert all(v == 0.0 for k, v in w.items() if k != q)
    assert not missed, missed


def test_sign_flip_on_axis_edges_is_caught():
    """On an axis edge all but a few entries of the l = 4 and l = 5 blocks vanish; flipping the
    sign of any surviving one (a wrong sign in a recursion table shows only through these) breaks
    the bound, on every axis edge at and inside the cutoff."""
    blk, vec, cls, cots, ref, f32 = _case(5, 2.0, 8, 5, "random")
    n = 0
    for e in torch.cat([cls["axis"], cls["cut_at"], cls["cut_in"]]).tolist():
        for l in (4, 5):
            alive = torch.nonzero(ref["sh"][e, l * l:(l + 1) ** 2].abs() > 1e-3).reshape(-1) + l * l
            assert 1 <= len(alive) <= 3, (e, l, alive)
            for j in alive.tolist():
                bad = {"sh": f32["sh"].clone()}
                bad["sh"][e, j] = -bad["sh"][e, j]
                w = k1_ref.compare(bad, vec, blk, 5, cots, ref, rows=torch.tensor([e]))
                assert w["sh"] > LOOSEST, (e, l, j, w)
                n += 1
    print(f"sign flips caught: {n}")


@pytest.mark.parametrize("lmax", [0, 1, 2, 3, 4, 5])
def test_block_norms_in_fp64(lmax):
    blk, vec, cls, cots, ref, _ = _case(lmax, 2.0, 8, 5, "random")
    rows = k1_ref.live_rows(vec)
    for l in range(lmax + 1):
        n2 = ref["sh"][rows, l * l:(l + 1) ** 2].pow(2).sum(-1)
        assert float((n2 - (2 * l + 1)).abs().max()) < 1e-12 * (2 * l + 1), l
    zero = ref["sh"][cls["zero"]]
    assert bool((zero[:, 0] == 1).all()) and not bool(zero[:, 1:].any())
