"""The host's rule for the block groups per tile of the index build's high-byte pass (index_tile_split in
csrc/k_hamming_index.hip, through hvd_index_tile_split; CPU test, host arithmetic only): G is 1, 2 or 4, a function of n and
the compute units alone -- so every rank of a pass derives the same grid --, never rises with n, is 1 from four workgroups
per compute unit on (where the launch is the one it was before the split: 10 M hashes on 256 compute units), and above 1
at 1 M hashes on 256 compute units, where 245 tiles leave compute units idle."""
import ctypes as C

import pytest

TILE = 4096


@pytest.fixture(scope="module")
def rule(hvd):
    from hvd_amd import _lib

    fn = _lib.load().hvd_index_tile_split  # (bound by hand: include/hvd_mi355x_bench.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_int64, C.c_int]
    return fn


def _sizes():
    edges = [k * TILE + d for k in (1, 2, 64, 127, 128, 129, 245, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2442) for d in (-1, 0, 1)]
    return sorted(set([1, 2, 1000, 1_000_000, 1 << 20, 2_000_000, 10_000_000, (1 << 32) - 1] + edges))


@pytest.mark.parametrize("cus", [1, 64, 104, 228, 256, 304])
def test_split_is_monotone_in_n_and_one_of_three(rule, cus):
    got = [rule(n, cus) for n in _sizes()]
    assert set(got) <= {1, 2, 4}, got
    assert all(a >= b for a, b in zip(got, got[1:])), list(zip(_sizes(), got))
    # one workgroup per tile from four workgroups per compute unit on, and not before
    assert rule(4 * cus * TILE - TILE + 1, cus) == 1 and rule(4 * cus * TILE - TILE, cus) > 1


def test_every_rank_derives_the_same_grid(rule):
    """Nothing but n and the compute units enters: the same call gives the same G, whoever asks and in whatever order."""
    asked = [(n, cus) for n in _sizes() for cus in (256, 304)]
    first = [rule(n, cus) for n, cus in asked]
    again = [rule(n, cus) for n, cus in reversed(asked)][::-1]
    assert first == again


def test_headline_and_config_4_on_256_compute_units(rule):
    assert rule(10_000_000, 256) == 1  # 2442 tiles: today's launch
    assert rule(1_000_000, 256) > 1    # 245 tiles
    assert rule(1 << 20, 256) > 1


def test_arguments_are_checked(rule):
    assert rule(-1, 256) < 0 and rule(1000, 0) < 0 and rule(1 << 32, 256) < 0
