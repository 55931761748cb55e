"""The schedule of the single-channel conv kernels (csrc/conv1d_thin.hip), on the CPU: the library loads without a GPU
and the grids and chunks are host arithmetic. Every case of tests/thin_cases.py is asked of the launchers' own functions
(through m2d_debug_thin_schedule) and must be in the regime it is named for - a forward wave walks `r` tiles and the
tiles do not divide among the waves evenly (both loop exits are taken), a backward block covers the stated chunk and a
sample's last block is partial. tests/test_gpu_thin_persistent.py runs these very cases against fp64 references; were
a grid or the chunk rule retuned, it would go on passing without entering the loops it is there for - this file fails
instead and names the case."""
import os

import pytest

from tests import thin_cases as C

pytestmark = pytest.mark.skipif(
    any(v in os.environ for v in ("M2D_THIN_WG_PER_CU", "M2D_THIN_LONG")),
    reason="M2D_THIN_WG_PER_CU / M2D_THIN_LONG is set: the library reads them once per process and the grids asked "
           "here would not be the default ones")


def _ceil(a, b):
    return -(-a // b)


def _check_forward(name, which, B, L, ks, stride, pad, tiles, r):
    got_tiles, waves, _ = C.schedule(which, B, L, ks, stride, pad)
    assert got_tiles == tiles, (name, got_tiles, tiles)
    assert waves > 0 and waves % 4 == 0, (name, waves)
    assert _ceil(tiles, waves) == r, "%s: %d tiles on %d waves are %d per wave, not %d" % (
        name, tiles, waves, _ceil(tiles, waves), r)
    assert tiles % waves != 0, "%s: every wave runs %d tiles - one of the loop's exits is never taken" % (name, r)


@pytest.mark.parametrize("case", C.K25_FWD_CASES, ids=lambda c: c[0])
def test_k25_forward_cases_walk_the_stated_tiles(case):
    name, B, L, ks, stride, pad, Lout, tiles, r = case
    assert C.out_len(L, ks, stride, pad) == Lout
    _check_forward(name, C.K25_FWD, B, L, ks, stride, pad, tiles, r)


@pytest.mark.parametrize("case", C.LONG_FWD_CASES, ids=lambda c: c[0])
def test_long_forward_cases_walk_the_stated_tiles(case):
    name, B, L, ks, stride, pad, Lout, tiles, r = case
    assert C.out_len(L, ks, stride, pad) == Lout
    _check_forward(name, C.LONG_FWD, B, L, ks, stride, pad, tiles, r)


@pytest.mark.parametrize("case", C.WINDOW_FWD_CASES, ids=lambda c: c[0])
def test_window_forward_cases_walk_the_stated_tiles(case):
    name, which, B, T, hop, window, ks, stride, pad, tiles, r = case
    _check_forward(name, which, B * T, window, ks, stride, pad, tiles, r)


def test_the_grids_are_the_ones_the_cases_were_worked_out_for():
    """4 096 waves for k25 and k160, 2 048 for k250, once there are that many tiles"""
    assert C.schedule(C.K25_FWD, 64, 76800, 25, 4, 11)[1] == 4096
    assert C.schedule(C.LONG_FWD, 7680, 3200, 250, 50, 124)[1] == 2048
    assert C.schedule(C.LONG_FWD, 7680, 3200, 160, 4, 79)[1] == 4096


def test_the_op_tests_of_test_gpu_kernels_give_a_wave_one_tile_at_most():
    """what this file's cases add: the largest single-channel shapes of tests/test_gpu_kernels.py stay inside one round"""
    for which, conv in ((C.K25_FWD, (2, 76800, 25, 4, 11)), (C.LONG_FWD, (40, 3200, 250, 50, 124)),
                        (C.LONG_FWD, (10, 3200, 160, 4, 79))):
        tiles, waves, _ = C.schedule(which, *conv)
        assert 0 < tiles <= waves, (conv, tiles, waves)
    for which in (C.BWD_WEIGHT, C.BWD_DATA):
        assert C.schedule(which, 2, 76800, 25, 4, 11)[1] == 1024


@pytest.mark.parametrize("which", [C.BWD_WEIGHT, C.BWD_DATA], ids=["bwd_weight", "bwd_data"])
@pytest.mark.parametrize("case", C.BWD_CASES, ids=lambda c: c[0])
def test_backward_cases_have_the_stated_chunk_and_a_partial_last_block(case, which):
    name, B, L, pad, Lout, chunk, blocks = case
    assert C.out_len(L, 25, 4, pad) == Lout
    n, got_chunk, got_blocks = C.schedule(which, B, L, 25, 4, pad)
    assert n == (Lout if which == C.BWD_WEIGHT else (L - 1 + pad) // 4 + 1), (name, n)
    assert got_chunk == chunk, "%s: chunk %d, not %d" % (name, got_chunk, chunk)
    assert got_chunk != 1024 and got_chunk % 256 == 0     # (whole rounds of a block's four waves)
    assert got_blocks == blocks == _ceil(n, chunk), (name, got_blocks, blocks)
    assert n % chunk != 0, "%s: the last block of a sample is whole" % name


def test_backward_data_leaves_a_wave_of_the_last_block_idle():
    """chunk-1536 in backward-data: 19 203 positions, 771 of them in the 13th block - a wave owns chunk / 4 = 384, so two
    waves are full, the third has 3 positions and the fourth none"""
    name, B, L, pad, Lout, chunk, blocks = C.BWD_CASES[0]
    n, got_chunk, got_blocks = C.schedule(C.BWD_DATA, B, L, 25, 4, pad)
    left = n - (got_blocks - 1) * got_chunk
    run = got_chunk // 4
    assert (n, left) == (19203, 771)
    assert 2 * run < left < 2 * run + 64 and left <= 3 * run


def test_convs_without_a_kernel_are_refused():
    assert C.schedule(C.K25_FWD, 4, 3200, 9, 1, 4) == (-1, -1, -1)
    assert C.schedule(C.LONG_FWD, 4, 3200, 25, 4, 11) == (-1, -1, -1)
    assert C.schedule(C.LONG_FWD, 4, 3202, 250, 50, 124) == (-1, -1, -1)     # (window no multiple of 4)
    assert C.schedule(C.BWD_WEIGHT, 4, 3200, 250, 50, 124) == (-1, -1, -1)
    assert C.schedule(7, 4, 3200, 25, 4, 11) == (-1, -1, -1)
