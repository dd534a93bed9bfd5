"""The launch arithmetic of the triplet kernels' gradient routes (csrc/gmp_sphbasis.hip,
csrc/gmp_tripletmp.hip), on the CPU: the *_partial_rows queries make no HIP call.

tests/test_gpu_triplet_routes.py runs each route at the smallest size that selects it and derives
the route from these queries; the thresholds themselves are pinned here, so a changed cap
(kProjBwdBlocks, kProjBwdBlocksAngleOnly, kBwdBlocks, kWaves, kTile, kEdgeT) shows up on a machine
without a GPU too.  The caps fix the order of the partial sums that the measured numbers of
DESIGN.md 7c / 7d rest on.

The expected numbers are worked out by hand from the constants as the launchers use them:
    triplet_proj_wgrad<kTorsion>: rows = max(1, min(ceil(T / 64), cap)), cap 512 with torsion and
        4096 without; tiles_per_block = ceil(ceil(T / 64) / rows)
    interact_bwd / interact1_bwd: rows = 4 max(1, min(ceil(E / 4), 2048)); epw = ceil(E / rows)
    edge_basis_bwd: rows = ceil(E / 256), 0 for E = 0
"""
import os

import pytest


def _lib_or_skip():
    from gmp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgmp.so not built")
    return _lib.load()


def _ceil_div(a, b):
    return -(-a // b)


# T: (rows, tiles per block, trailing blocks that own no tile)
SPH_PROJ = {
    0: (1, 0, 1), 1: (1, 1, 0), 64: (1, 1, 0), 65: (2, 1, 0),
    32_704: (511, 1, 0), 32_705: (512, 1, 0),
    32_768: (512, 1, 0),      # the last size with one tile per block
    32_769: (512, 2, 255),    # 513 tiles: blocks 0..256 busy (the last with one tile)
    37_271: (512, 2, 220),    # the list of test_gpu_triplet_routes
    65_536: (512, 2, 0), 65_537: (512, 3, 170),
    3_536_644: (512, 108, 0),  # the workload of DESIGN.md 7c: 55,261 tiles
}
DIME_PROJ = {
    0: (1, 0, 1), 1: (1, 1, 0), 65: (2, 1, 0), 32_769: (513, 1, 0), 37_271: (583, 1, 0),
    262_144: (4096, 1, 0),    # the last size with one tile per block
    262_145: (4096, 2, 2047),
    262_209: (4096, 2, 2047),  # 4096 * 64 + 65, test_dimenet_wgrad_cap
    3_536_644: (4096, 14, 148),
}
# E: (rows, edges per wave, trailing waves that own no edge), K19 and K19d alike
INTERACT = {
    0: (4, 0, 4), 1: (4, 1, 3), 4: (4, 1, 0), 5: (8, 1, 3), 300: (300, 1, 0),
    8_192: (8192, 1, 0),      # the last size with one edge per wave
    8_193: (8192, 2, 4095),
    8_257: (8192, 2, 4063),   # the list of test_gpu_triplet_routes
    16_384: (8192, 2, 0), 16_385: (8192, 3, 2730),
    263_600: (8192, 33, 204),  # the workload of DESIGN.md 7c / 7d
}
EDGE_BASIS = {0: 0, 1: 1, 256: 1, 257: 2, 500: 2, 8_257: 33, 263_600: 1030}


def _route(rows, units):
    per = _ceil_div(units, rows)
    return rows, per, rows - (_ceil_div(units, per) if per else 0)


@pytest.mark.parametrize("name,table", [("gmp_sph_triplet_proj_bwd_partial_rows", SPH_PROJ),
                                        ("gmp_dime_triplet_proj_bwd_partial_rows", DIME_PROJ)])
def test_proj_wgrad_routes(name, table):
    lib = _lib_or_skip()
    got = {T: _route(getattr(lib, name)(T), _ceil_div(T, 64)) for T in table}
    assert got == table


@pytest.mark.parametrize("name", ["gmp_triplet_interact_bwd_partial_rows",
                                  "gmp_triplet_interact1_bwd_partial_rows"])
def test_interact_bwd_routes(name):
    lib = _lib_or_skip()
    got = {E: _route(getattr(lib, name)(E), E) for E in INTERACT}
    assert got == INTERACT


@pytest.mark.parametrize("name", ["gmp_sph_edge_basis_bwd_partial_rows",
                                  "gmp_dime_edge_basis_bwd_partial_rows"])
def test_edge_basis_bwd_rows(name):
    lib = _lib_or_skip()
    assert {E: getattr(lib, name)(E) for E in EDGE_BASIS} == EDGE_BASIS


def test_thresholds_are_where_the_gpu_module_runs():
    """The sizes test_gpu_triplet_routes uses sit past each threshold, with idle trailing blocks /
    waves, and the workload's own sizes take the same routes."""
    assert SPH_PROJ[32_768][1] == 1 and SPH_PROJ[32_769][1] == 2
    assert DIME_PROJ[262_144][1] == 1 and DIME_PROJ[262_145][1] == 2
    assert INTERACT[8_192][1] == 1 and INTERACT[8_193][1] == 2
    for table, size in ((SPH_PROJ, 37_271), (DIME_PROJ, 262_209), (INTERACT, 8_257)):
        rows, per, idle = table[size]
        assert per >= 2 and idle >= 1
    assert SPH_PROJ[3_536_644][1] >= 2 and DIME_PROJ[3_536_644][1] >= 2
    assert INTERACT[263_600][1] >= 2
