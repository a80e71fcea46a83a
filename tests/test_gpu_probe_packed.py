"""The probe of an index-eligible self pass on the packed hashes (k_prefilter_probe_packed in csrc/k_hamming_mfma.hip) against
the image probe it replaces there (k_prefilter_probe, "mfma_probe_packed" 0) and against the host model
(tests/tools/probe_ref.py): the six words the probe leaves -- form, lo, hi, selection, mix, close -- are the same integers
whichever kernel counted them, and the pair list is the oracle's both times.

Sizes: the smallest that reach every edge of the sampling -- a column block with fewer than 64 live columns (2, 63, 65), an
exact one (64), lanes past the last sample row (257), stride 1 with more rows than one grid row (4097), stride 2 (8192),
stride 3 with the half-stride column offset clamped at n - 1 (12289). Tolerances: 0, 1, 15 (block radius 0) and 16, 31
(radius 1). Libraries: probe_ref's near copies, uniform hashes, frame-like clusters, and a planted library whose pairs differ
in exactly 0, 1 or 2 bits per 16-bit half -- bit 0, 15, 16 or 31 alone, one bit in either half, two in one -- the inputs on
which arithmetic that let a borrow or a minimum cross from one half into the other would count another `close`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cross_ref  # noqa: E402
import probe_ref  # noqa: E402
from test_gpu_probe import _cross_pass, _self_pass  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (2, 63, 64, 65, 257, 4097, 8192, 12289)
TOLERANCES = (0, 1, 15, 16, 31)


class _Knobs:
    """hvd_debug_set with the defaults restored however the block ends."""

    DEFAULTS = {b"allpairs_index": -1, b"mfma_probe_packed": 1}

    def __init__(self, gpu, **kv):
        self.lib, self.gpu, self.kv = gpu.load(), gpu, {k.encode(): v for k, v in kv.items()}

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                self.gpu.check(self.lib.hvd_debug_set(k, v))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            self.gpu.check(self.lib.hvd_debug_set(k, self.DEFAULTS[k]))


def _image_then_packed(gpu, hvd, oracle, db, max_dist):
    """The index-branch self pass with the image probe and then with the packed one: equal words, the model's counts, the
    oracle's pairs (checked inside _self_pass) both times."""
    want = oracle.allpairs(db, max_dist, num_threads=8, cap=1 << 20)
    ref = probe_ref.counts(db, db, max_dist, probe_ref.index_radius(max_dist))
    with _Knobs(gpu, allpairs_index=1, mfma_probe_packed=0):
        image = _self_pass(gpu, hvd, db, want, max_dist)
    with _Knobs(gpu, allpairs_index=1, mfma_probe_packed=1):
        packed = _self_pass(gpu, hvd, db, want, max_dist)
    assert image.index_used == 1 and packed.index_used == 1
    assert packed.words == image.words, (len(db), max_dist)
    assert packed.counts + (packed.close,) == ref, (len(db), max_dist, packed.words, ref)
    return packed


# ------------------------------------------------------------------ the sampling's edges, at every tolerance

@pytest.mark.parametrize("max_dist", TOLERANCES)
@pytest.mark.parametrize("n", SIZES)
def test_same_words_from_either_probe(gpu, hvd, oracle, n, max_dist):
    _image_then_packed(gpu, hvd, oracle, probe_ref.near_copy_library(n, n), max_dist)


# ------------------------------------------------------------------ libraries that exercise the packed arithmetic

@pytest.mark.parametrize("max_dist", TOLERANCES)
def test_uniform_hashes(gpu, hvd, oracle, max_dist):
    db = np.random.default_rng(4097).integers(0, 256, (4097, 32), dtype=np.uint8)
    _image_then_packed(gpu, hvd, oracle, db, max_dist)


@pytest.mark.parametrize("max_dist", TOLERANCES)
def test_clustered_hashes(gpu, hvd, oracle, max_dist):
    """60 clusters of 20 near-identical hashes in 9000 (stride 2): 50 753 sampled blocks at distance 0, 139 735 within 1."""
    from hvd_amd import synth
    db, _ = synth.hash_db_clustered(9000, 60, 20, seed=8)
    p = _image_then_packed(gpu, hvd, oracle, db, max_dist)
    assert p.close == (139735 if max_dist >= 16 else 50753)


# word masks of the planted pairs: (low half's bits, high half's bits) flipped
MASKS = {
    "bit0": 0x00000001, "bit15": 0x00008000, "bit16": 0x00010000, "bit31": 0x80000000,       # 1 | 0 and 0 | 1
    "low2": 0x00000003, "low2_top": 0x0000C000, "high2": 0x00030000, "high2_top": 0xC0000000,  # 2 | 0 and 0 | 2
    "one_one": 0x00010001, "one_one_outer": 0x80000001, "one_one_inner": 0x00018000, "one_one_top": 0x80008000,  # 1 | 1
    "two_one": 0x00010003, "one_two": 0x00030001, "two_two": 0x00030003,                      # 2 | 1, 1 | 2, 2 | 2
}
PLANTED_N = 300  # stride 1: the sample is every ordered pair; two grid rows, five column blocks (the last with 44 columns)


def _halves_beyond(mask, r):
    return int(bin(mask & 0xFFFF).count("1") > r) + int(bin(mask >> 16).count("1") > r)


@pytest.fixture(scope="module")
def planted():
    """Row 2k + 1 = row 2k with the k-th mask (MASKS in order, each in words 0..7 in turn) XORed in: fifteen of the pair's
    blocks at distance 0, the last two as the mask says. Before any device run, on the CPU: probe_ref.counts sees every one
    of these cases -- over the two rows alone (n = 2 samples both rows against both) `close` is the diagonal's 32 blocks plus,
    in either order of the pair, the 16 blocks less the mask's halves beyond the radius, so each mask with such a half
    changes the total against an exact copy, and every mask does at radius 0."""
    db = np.random.default_rng(23).integers(0, 256, (PLANTED_N, 32), dtype=np.uint8)
    words = db.view("<u4")
    k = 0
    for name, mask in MASKS.items():
        for w in range(8):
            words[2 * k + 1] = words[2 * k]
            words[2 * k + 1, w] ^= np.uint32(mask)
            two = db[2 * k:2 * k + 2]
            for r, max_dist in ((0, 15), (1, 31)):
                assert probe_ref.counts(two, two, max_dist, r)[3] == 32 + 2 * (16 - _halves_beyond(mask, r)), (name, w, r)
            k += 1
    assert 2 * k <= PLANTED_N
    assert all(_halves_beyond(m, 0) > 0 for m in MASKS.values())
    assert {_halves_beyond(m, 1) for m in MASKS.values()} == {0, 1, 2}
    return db


@pytest.mark.parametrize("max_dist", TOLERANCES)
def test_planted_halves_of_zero_one_and_two_bits(gpu, hvd, oracle, planted, max_dist):
    _image_then_packed(gpu, hvd, oracle, planted, max_dist)


# ------------------------------------------------------------------ determinism, and where the packed probe does not run

def test_the_same_words_on_every_repetition(gpu, hvd, oracle):
    """Twice in a row, and once more behind an unrelated pass: the words are cleared per launch and the ticket counts
    exactly one last workgroup."""
    db = probe_ref.near_copy_library(3001, 3001)
    other = probe_ref.near_copy_library(8192, 8192)
    want, want_other = oracle.allpairs(db, 31), oracle.allpairs(other, 31)
    with _Knobs(gpu, allpairs_index=1, mfma_probe_packed=1):
        first = _self_pass(gpu, hvd, db, want).words
        assert _self_pass(gpu, hvd, db, want).words == first
        assert _self_pass(gpu, hvd, other, want_other).words != first
        assert _self_pass(gpu, hvd, db, want).words == first
    assert first[1:3] + first[4:6] == probe_ref.counts(db, db, 31, 1)


def test_the_knob_changes_nothing_without_the_index_or_across_two_sets(gpu, hvd, oracle):
    """Index off: the image probe's first branch whatever the knob says, close == 0. The cross entry never passes an index
    radius: the same."""
    db = probe_ref.near_copy_library(4097, 4097)
    want = oracle.allpairs(db, 31)
    q, t = probe_ref.near_copy_sets(300, 8200, 300 * 7919 + 8200)
    want_x = cross_ref.cross_oracle(oracle, q, t, 31)
    words, words_x = [], []
    for packed in (0, 1):
        with _Knobs(gpu, allpairs_index=0, mfma_probe_packed=packed):
            p = _self_pass(gpu, hvd, db, want)
            assert p.close == 0 and p.index_used == 0 and p.counts == probe_ref.counts(db, db, 31)
            words.append(p.words)
        with _Knobs(gpu, mfma_probe_packed=packed):
            x = _cross_pass(gpu, hvd, q, t, want_x)
            assert x.close == 0 and x.index_used == 0 and x.counts == probe_ref.counts(q, t, 31)
            words_x.append(x.words)
    assert words[0] == words[1] and words_x[0] == words_x[1]
