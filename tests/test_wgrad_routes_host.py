"""The outer-sum dispatcher's route table (gmp_edge_outer_sum_ex_route, csrc/gmp_wgrad.hip), on
the CPU: the query makes no HIP call, and gmp_edge_outer_sum_ex_f32 returns before any HIP call
wherever the route is the library GEMM or the arguments are invalid.

The table below was evaluated by hand from the dispatcher as it stood before the query existed
(the argument checks, x3 / quadrant / bucket tests and their order in outer_sum_launch and
outer_sum_rect_launch), not copied from the query's output.  It differs from that dispatcher
only where it returned GMP_ERR_ARG (-1) for a valid shape, because
`GMP_CHECK_ARG(m <= kT || quad_ok(...))` stood in front of the GMP_ERR_UNSUPPORTED return; those
rows are LIBRARY now (gmp_edge_outer_sum_ex_f32 returns -3 and the op runs the library GEMM).
In both modes of gmp_wgrad_set_f32_mfma:
    320 x 64, 576 x 192, 1024 x 1024   at K in {0, 262144, 262145, 1000003}
    1088 x 64, 272 x 16                at every K
"""
import ctypes
import os

import pytest

KS = (0, 1, 255, 256, 262_143, 262_144, 262_145, 1_000_003)
# one letter per K of KS
CODE = {"Z": "ZERO", "X": "X3", "Q": "QUAD", "S": "SQUARE_F32", "R": "RECT_F32", "L": "LIBRARY",
        "A": "ARG"}
# (m, n, lda): routes in split-plane mode (gmp_wgrad_set_f32_mfma(0)), in f32-MFMA mode (1)
TABLE = {
    (32, 32, 32):       ("ZSSSSSSS", "ZSSSSSSS"),
    (64, 64, 64):       ("ZQQQQXXX", "ZQQQQSSS"),
    (128, 128, 128):    ("ZQQQQXXX", "ZQQQQSSS"),
    (16, 128, 16):      ("ZRRRRRRR", "ZRRRRRRR"),   # m n < 4096: never the split planes
    (128, 16, 128):     ("ZRRRRRRR", "ZRRRRRRR"),
    (48, 144, 48):      ("ZRRRRXXX", "ZRRRRRRR"),
    (128, 144, 128):    ("ZRRRRXXX", "ZRRRRRRR"),
    (128, 256, 128):    ("LQQQQLLL", "LQQQQLLL"),   # m + n > 288: no bucket, no x3 tiling
    (256, 64, 256):     ("LQQQQLLL", "LQQQQLLL"),
    (320, 64, 320):     ("LQQQQLLL", "LQQQQLLL"),
    (576, 192, 576):    ("LQQQQLLL", "LQQQQLLL"),   # K17: [s | vn]^T dspre
    (192, 576, 192):    ("LQQQQLLL", "LQQQQLLL"),   # K17
    (192, 64, 192):     ("ZQQQQXXX", "ZQQQQRRR"),   # K17
    (192, 128, 192):    ("LQQQQLLL", "LQQQQLLL"),   # K17
    (1024, 1024, 1024): ("LQQQQLLL", "LQQQQLLL"),
    (1088, 64, 1088):   ("LLLLLLLL", "LLLLLLLL"),   # m > 1024
    (272, 16, 272):     ("LLLLLLLL", "LLLLLLLL"),   # m > 256, not a multiple of 64
    (128, 144, 148):    ("ZRRRRXXX", "ZRRRRRRR"),   # valid stride
    (128, 144, 146):    ("AAAAAAAA", "AAAAAAAA"),   # lda % 4 != 0
}


def _lib_or_skip():
    from gmp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmp.so not built")
    return _lib, _lib.load()


def _value(_lib, name):
    return _lib.GMP_ERR_ARG if name == "ARG" else getattr(_lib, "WGRAD_ROUTE_" + name)


def test_route_enum_matches_header():
    import re
    from conftest import ROOT
    from gmp_amd import _lib
    txt = open(os.path.join(ROOT, "include", "gmp.h")).read()
    found = dict(re.findall(r"GMP_WGRAD_ROUTE_([A-Z0-9_]+) = (\d+)", txt))
    assert sorted(found) == sorted(n for n in CODE.values() if n != "ARG")
    for name, val in found.items():
        assert getattr(_lib, "WGRAD_ROUTE_" + name) == int(val)


def test_route_table():
    _lib, lib = _lib_or_skip()
    prev = lib.gmp_wgrad_set_f32_mfma(0)
    bad = []
    try:
        for mode in (0, 1):
            lib.gmp_wgrad_set_f32_mfma(mode)
            for (m, n, lda), rows in TABLE.items():
                assert len(rows[mode]) == len(KS)
                for K, letter in zip(KS, rows[mode]):
                    want = _value(_lib, CODE[letter])
                    got = lib.gmp_edge_outer_sum_ex_route(K, m, n, lda, n, -1)
                    if got != want:
                        bad.append((mode, K, m, n, lda, CODE[letter], got))
                    if letter not in "LA":
                        continue
                    # no kernel and no zero fill: the call returns before any HIP call, with
                    # the query's decision (null data pointers, no workspace)
                    rc = lib.gmp_edge_outer_sum_ex_f32(K, m, n, None, lda, None, n, -1, None,
                                                       None, None, n, None, None, 0, None)
                    want_rc = _lib.GMP_ERR_UNSUPPORTED if letter == "L" else _lib.GMP_ERR_ARG
                    if rc != want_rc:
                        bad.append((mode, K, m, n, lda, "ex_f32 returns", rc))
    finally:
        lib.gmp_wgrad_set_f32_mfma(prev)
    assert not bad, bad


def test_route_invalid_arguments_and_activation():
    """Invalid sizes are GMP_ERR_ARG in the query and in the call; the activation prologue exists
    for the square kernel's shapes only (elsewhere: LIBRARY)."""
    _lib, lib = _lib_or_skip()
    route = lib.gmp_edge_outer_sum_ex_route
    for K, m, n, lda, ldb, act in [(-1, 128, 144, 128, 144, -1), (5, 0, 16, 16, 16, -1),
                                   (5, 24, 16, 24, 16, -1), (5, 16, 40, 16, 40, -1),
                                   (5, 128, 144, 112, 144, -1), (5, 128, 144, 128, 128, -1),
                                   (5, 128, 144, 128, 146, -1), (5, 128, 128, 130, 128, -1),
                                   (-1, 64, 64, 64, 64, 0), (5, 64, 64, 64, 64, 2),
                                   (5, 64, 64, 64, 64, -2)]:
        assert route(K, m, n, lda, ldb, act) == _lib.GMP_ERR_ARG, (K, m, n, lda, ldb, act)
        assert lib.gmp_edge_outer_sum_ex_f32(K, m, n, None, lda, None, ldb, act, None, None, None,
                                             n, None, None, 0, None) == _lib.GMP_ERR_ARG
    prev = lib.gmp_wgrad_set_f32_mfma(0)
    try:
        for act in (0, 1):
            assert route(300_000, 128, 128, 128, 128, act) == _lib.WGRAD_ROUTE_X3
            assert route(5, 128, 128, 128, 128, act) == _lib.WGRAD_ROUTE_SQUARE_F32  # no quad
            assert route(0, 64, 64, 64, 64, act) == _lib.WGRAD_ROUTE_ZERO
            assert route(5, 128, 144, 128, 144, act) == _lib.WGRAD_ROUTE_LIBRARY
        lib.gmp_wgrad_set_f32_mfma(1)
        assert route(300_000, 128, 128, 128, 128, 0) == _lib.WGRAD_ROUTE_SQUARE_F32
    finally:
        lib.gmp_wgrad_set_f32_mfma(prev)


def test_library_routes_need_no_workspace():
    _lib, lib = _lib_or_skip()
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    for K in (0, 262_144):
        assert lib.gmp_edge_outer_sum_ex_workspace_size(K, 576, 192) == 0
        assert lib.gmp_edge_outer_sum_ex_workspace_size(K, 272, 16) == 0
