"""nu_gemm_nt_tile_rows: which row-tile height (64 or 128) an exact-fp32 NT GEMM launch takes.  A host function: no GPU, no launch.

The table was computed from the rule's definition, independently of the library (column tiles of 128; t128 / t64 = row tiles of 128 /
64 rows x column tiles x groups; efficiency of a tile count = tiles / (ceil(tiles / 512) * 512); 64-row tiles when t128 < 512 or
0.95 * efficiency(t64) > efficiency(t128)).  The GPU tests assert the height they mean to exercise with the same entry, so a change
of the rule that moves a test off its kernel shows up here and there."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from nu_nerf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _problem(M, N, K=32, groups=1, epi=7, **kw):
    from nu_nerf_amd._lib import GemmNT
    return GemmNT(lda=K, ldb=K, M=M, N=N, K=K, ldc=N, alpha=1.0, groups=groups, epi=epi, **kw)


def _rule(M, N, groups):
    """The rule as the header of this file states it, in integers and fractions only."""
    from fractions import Fraction
    ntn = -(-N // 128)
    t128, t64 = -(-M // 128) * ntn * groups, -(-M // 64) * ntn * groups
    eff = lambda t: Fraction(t, -(-t // 512) * 512)
    return 64 if t128 < 512 or Fraction(95, 100) * eff(t64) > eff(t128) else 128


TABLE = [(66048, 256, 1, 64), (65990, 384, 1, 64), (4099, 256, 1, 64), (40000, 128, 1, 64), (22000, 340, 1, 64), (11000, 256, 4, 64),
         (262144, 256, 1, 128), (8192, 256, 4, 128), (8155, 256, 4, 128), (65500, 128, 1, 128), (16300, 512, 1, 128), (32700, 256, 1, 128),
         (64000, 256, 1, 128), (63990, 384, 1, 128)]


@pytest.mark.parametrize("M,N,groups,rows", TABLE)
def test_tile_rows_table(lib, M, N, groups, rows):
    assert _rule(M, N, groups) == rows                       # the table agrees with its own definition
    for epi in range(9):
        g = _problem(M, N, groups=groups, epi=epi)
        assert lib.nu_gemm_nt_tile_rows(ctypes.byref(g), 1) == rows, epi


def test_tile_rows_follows_the_rule_over_a_sweep(lib):
    for M in (1, 64, 65, 4096, 8191, 16384, 16385, 30000, 32768, 33000, 50000, 65536, 66048, 70000, 131072, 200000, 527000):
        for N in (1, 128, 129, 256, 340, 384, 512, 1024):
            for groups in (1, 2, 4):
                g = _problem(M, N, groups=groups)
                assert lib.nu_gemm_nt_tile_rows(ctypes.byref(g), 1) == _rule(M, N, groups), (M, N, groups)


def test_tile_rows_other_modes_empty_launches_and_errors(lib):
    from nu_nerf_amd._lib import GemmNT, NuNerfLibraryError
    big = dict(M=262144, N=256)
    for mode in (1, 2):                                      # bf16 and bf16x6 arithmetic: another kernel
        g = _problem(**big, bf16=mode)
        assert lib.nu_gemm_nt_tile_rows(ctypes.byref(g), 1) == 0
    assert lib.nu_gemm_nt_tile_rows(ctypes.byref(_problem(0, 256)), 1) == 0        # M == 0 launches nothing
    assert lib.nu_gemm_nt_tile_rows(None, 0) == 0
    for bad in (_problem(**big, K=48), _problem(**big, epi=9), _problem(**big, bf16=3), GemmNT(lda=30, ldb=32, K=32, **big)):
        with pytest.raises(NuNerfLibraryError, match="nu_gemm_nt_tile_rows failed with code -1"):
            lib.nu_gemm_nt_tile_rows(ctypes.byref(bad), 1)
    with pytest.raises(NuNerfLibraryError, match="code -1"):
        lib.nu_gemm_nt_tile_rows(None, 2)
    with pytest.raises(NuNerfLibraryError, match="code -1"):
        lib.nu_gemm_nt_tile_rows(ctypes.byref(_problem(**big)), -1)


def test_tile_rows_of_a_batch_is_that_of_its_first_run(lib):
    """nu_gemm_nt_batch sums the tiles of the run that shares a launch: problems of one epilogue kind that has a batch build
    (0, 1, 3, 7), exact fp32, at most NU_NT_BATCH_MAX after group expansion; empty problems are skipped."""
    from nu_nerf_amd._lib import GemmNT

    def rows(*probs):
        return lib.nu_gemm_nt_tile_rows((GemmNT * len(probs))(*probs), len(probs))
    eight = [_problem(M, 256) for M in (8155, 8192, 8100, 8129, 8065, 8190, 8180, 8170)]
    assert rows(*eight) == 128                               # 8 x 64 x 2 = 1024 tiles of 128 rows: two full rounds
    assert rows(*eight[:3]) == 64                            # 384 tiles: fewer than 512
    assert rows(_problem(8155, 256)) == 64 and rows(_problem(8155, 256, groups=4)) == 128
    assert rows(*eight, _problem(100, 64)) == 128            # the ninth problem opens a second run
    assert rows(_problem(0, 256), *eight) == 128             # an empty problem takes no slot of the run
    # a change of epilogue ends the run: one problem is a single launch, decided on its own tiles
    assert rows(_problem(262144, 256, epi=0), _problem(100, 256, epi=7)) == 128
    assert rows(_problem(100, 256, epi=0), _problem(262144, 256, epi=7)) == 64
    # epilogues without a batch build fall through to single launches
    assert rows(_problem(262144, 256, epi=2), _problem(262144, 256, epi=2)) == 128
    assert rows(_problem(100, 256, epi=4), _problem(262144, 256, epi=4)) == 64
    # a run of the other arithmetic modes is a single launch of another kernel
    assert rows(_problem(262144, 256, bf16=1), _problem(262144, 256, bf16=1)) == 0


def test_tile_rows_of_the_shapes_the_128_row_test_uses(lib):
    """tests/test_gemm_gpu.py::test_epilogue_fast_path_copies_on_128_row_tiles launches N = 256 and N = 384 at two row counts, the
    second with a ragged last tile: both must be 128-row launches (the row counts it used before were not)."""
    for M in (64000, 63990):
        for N in (256, 384):
            assert lib.nu_gemm_nt_tile_rows(ctypes.byref(_problem(M, N, K=64)), 1) == 128
    for M in (66048, 65990):
        for N in (256, 384):
            assert lib.nu_gemm_nt_tile_rows(ctypes.byref(_problem(M, N, K=64)), 1) == 64
