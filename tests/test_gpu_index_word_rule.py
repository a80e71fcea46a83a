"""The index join's word rule on the GPU (csrc/k_hamming_index.hip: first stage on the 32-bit word that holds the block,
survivor queue, ownership by the lowest QUALIFYING block), index forced ("allpairs_index" 1): every pair list equals the CPU
oracle's and holds no pair twice. Random hashes with planted pairs; what each planted pair is (distance, qualifying blocks)
is asserted with the numpy model of index_word_helpers.py before the GPU sees it.

A pair "whose only qualifying word is w, with that word at exactly tw" needs tw + 1 differing bits in each of the other
seven words, 8 tw + 7 in all: that fits distance max_dist only for max_dist = 7, 15, 23, 31 (and max_dist + 1 for none but
those and 8 tw + 6). For the other max_dist the remaining bits make as many of the other words fail as they reach; the
model says which blocks qualify, and the test asserts "only word w" exactly where the arithmetic allows it."""
import ctypes as C

import numpy as np
import pytest

import index_word_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture
def forced(gpu):
    gpu.check(gpu.load().hvd_debug_set(b"allpairs_index", 1))
    yield
    gpu.check(gpu.load().hvd_debug_set(b"allpairs_index", -1))


def _check(hvd, gpu, oracle, db, md, group=None):
    want = oracle.allpairs(db, md, group=group)
    got = hvd.allpairs_hamming(db, md, group=group)
    used = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(b"allpairs_index_used", C.byref(used)))
    assert used.value == 1
    ids = got["i"].astype(np.int64) << 32 | got["j"].astype(np.int64)
    assert len(np.unique(ids)) == len(ids), "a pair occurs twice"
    assert np.array_equal(got, want), (len(got), len(want))
    return set(zip(want["i"].tolist(), want["j"].tolist()))


def _assemble(rng, planted, filler):
    """planted rows first (pair k = rows 2k, 2k + 1), then random filler, all shuffled; returns db and the rows' new places."""
    db = np.concatenate([np.array(planted, dtype=np.uint8).reshape(-1, 32), rng.integers(0, 256, (filler, 32), dtype=np.uint8)])
    perm = rng.permutation(len(db))
    where = np.empty(len(db), dtype=np.int64)
    where[perm] = np.arange(len(db))
    return db[perm], where


def _has(have, where, a, b):
    i, j = int(where[a]), int(where[b])
    return (min(i, j), max(i, j)) in have


@pytest.mark.parametrize("max_dist", H.MAX_DISTS)
def test_pairs_at_the_word_boundary_in_word_0_and_word_7(hvd, gpu, oracle, forced, max_dist):
    rng = np.random.default_rng(500 + max_dist)
    tw, r = H.tw_r(max_dist)
    rows, expect = [], []
    for w in (0, 7):
        for b in (2 * w, 2 * w + 1):  # the even, then the odd block carries e_b; the sibling sits at exactly tw - e_b
            for e_b in range(r + 1):
                for total in (max_dist, max_dist + 1):
                    for _ in range(6):
                        x = rng.integers(0, 256, 32, dtype=np.uint8)
                        y = H.partner(rng, x, b, e_b, tw - e_b, total, at_least=tw + 1) if total >= tw else None
                        if y is None:
                            continue
                        q = H.qualifying(x, y, max_dist)
                        assert q[b] and H.block_errors(x, y)[b ^ 1] == tw - e_b
                        if total - tw >= 7 * (tw + 1):
                            assert not q[[k for k in range(16) if k >> 1 != w]].any()  # only word w qualifies
                        expect.append((len(rows), len(rows) + 1, total <= max_dist))
                        rows += [x, y]
    db, where = _assemble(rng, rows, 2000)
    assert 2000 <= len(db) <= 9000
    have = _check(hvd, gpu, oracle, db, max_dist)
    for a, b, within in expect:
        assert _has(have, where, a, b) == within


@pytest.mark.parametrize("max_dist", [1, 7, 8, 15, 16, 23, 24, 31])
def test_a_block_within_r_whose_word_fails_does_not_own_the_pair(hvd, gpu, oracle, forced, max_dist):
    """Block b_lo of word 0: keys within r, its word beyond tw (e.g. e_b = 1 with the sibling at 3 for max_dist 31); the
    pair qualifies only in later words. The former ownership rule (lowest block with keys within r) would lose every one."""
    rng = np.random.default_rng(600 + max_dist)
    tw, r = H.tw_r(max_dist)
    rows = []
    for k in range(120):
        b_lo, w_hi = int(rng.integers(0, 2)), int(rng.integers(1, 8))
        x = rng.integers(0, 256, 32, dtype=np.uint8)
        y = x.copy()
        H.flip_in_block(rng, y, b_lo, r)
        H.flip_in_block(rng, y, b_lo ^ 1, tw + 1 - r)
        e_hi = int(rng.integers(0, tw + 1))
        H.flip_in_word(rng, y, w_hi, e_hi)
        left = max_dist - (tw + 1) - e_hi
        if k % 2 and left > 0:  # more bits outside the two words: whatever else qualifies lies behind word 0
            H.spread_over_words(rng, y, [w for w in range(8) if w not in (b_lo >> 1, w_hi)], int(rng.integers(0, left + 1)), tw + 1)
        assert int(H.popc(x ^ y).sum()) <= max_dist
        q = H.qualifying(x, y, max_dist)
        assert not q[b_lo] and not q[b_lo ^ 1] and q[2 * w_hi:2 * w_hi + 2].any()
        assert H.emitting_blocks(x, y, max_dist).sum() == 1 and H.old_rule_emitting_blocks(x, y, max_dist).sum() == 0
        rows += [x, y]
    db, where = _assemble(rng, rows, 2000)
    have = _check(hvd, gpu, oracle, db, max_dist)
    for k in range(0, len(rows), 2):
        assert _has(have, where, k, k + 1)


@pytest.mark.parametrize("with_group", [False, True])
def test_pairs_that_qualify_in_two_blocks_come_out_once(hvd, gpu, oracle, forced, with_group):
    rng = np.random.default_rng(7)
    rows, kinds = [], []
    for k in range(300):
        x = rng.integers(0, 256, 32, dtype=np.uint8)
        y = x.copy()
        if k % 2 == 0:  # both blocks of one word
            w = int(rng.integers(0, 8))
            H.flip_in_block(rng, y, 2 * w, int(rng.integers(0, 2)))
            H.flip_in_block(rng, y, 2 * w + 1, int(rng.integers(0, 2)))
            H.spread_over_words(rng, y, [v for v in range(8) if v != w], 28, 4)
            want = [2 * w, 2 * w + 1]
        else:  # one block in each of two words
            w1, w2 = sorted(int(v) for v in rng.choice(8, size=2, replace=False))
            b1, b2 = 2 * w1 + int(rng.integers(0, 2)), 2 * w2 + int(rng.integers(0, 2))
            H.flip_in_block(rng, y, b1, 1)
            H.flip_in_block(rng, y, b1 ^ 1, 2)
            H.flip_in_block(rng, y, b2, 1)
            H.flip_in_block(rng, y, b2 ^ 1, 2)
            H.spread_over_words(rng, y, [v for v in range(8) if v not in (w1, w2)], 24, 4)
            want = [b1, b2]
        assert np.flatnonzero(H.qualifying(x, y, 31)).tolist() == want and int(H.popc(x ^ y).sum()) <= 31
        rows += [x, y]
        kinds.append(want)
    db, where = _assemble(rng, rows, 2000)
    group = None
    if with_group:
        group = np.arange(len(db), dtype=np.int32)
        for k in range(0, 300, 3):  # every third planted pair shares a group: removed
            group[where[2 * k + 1]] = group[where[2 * k]]
    have = _check(hvd, gpu, oracle, db, 31, group=group)
    for k in range(300):
        assert _has(have, where, 2 * k, 2 * k + 1) == (not with_group or k % 3 != 0)


def test_every_same_bucket_candidate_survives_and_none_is_a_pair(hvd, gpu, oracle, forced):
    rng = np.random.default_rng(8)
    db = rng.integers(0, 256, (2300, 32), dtype=np.uint8)
    rows = rng.choice(2300, size=300, replace=False)
    db[rows, :4] = db[rows[0], :4]  # word 0 shared, the rest random: 44 850 survivors in block 0, as many in block 1
    assert len(np.unique(db[rows], axis=0)) == 300
    have = _check(hvd, gpu, oracle, db, 31)
    assert len(have) == 0


def test_identical_hashes_drain_the_queue_and_flush_the_pair_buffer_together(hvd, gpu, oracle, forced):
    rng = np.random.default_rng(9)
    db = rng.integers(0, 256, (2200, 32), dtype=np.uint8)
    rows = rng.choice(2200, size=200, replace=False)
    db[rows] = db[rows[0]]
    for md in (31, 0):
        assert len(_check(hvd, gpu, oracle, db, md)) == 19900


@pytest.mark.parametrize("length", [63, 64, 65, 129])
def test_y_lists_in_which_every_entry_survives(hvd, gpu, oracle, forced, length):
    """`length` hashes share word w (both its blocks: every candidate of those two buckets survives); the other seven
    words of member m differ from the first member's in (7 m) mod 41 bits, so pairs and non-pairs mix."""
    rng = np.random.default_rng(length)
    w = length % 8
    first = rng.integers(0, 256, 32, dtype=np.uint8)
    rows = []
    for m in range(length):
        y = first.copy()
        H.spread_over_words(rng, y, [v for v in range(8) if v != w], (7 * m) % 41, 0)
        rows.append(y)
    db, where = _assemble(rng, rows, 2000)
    keys = np.ascontiguousarray(db).view("<u2")
    filler = np.ones(len(db), dtype=bool)
    filler[where[:length]] = False
    for b in (2 * w, 2 * w + 1):  # the y list is the bucket alone: no filler row in it or one bit from it
        key = np.uint16(np.array(first).view("<u2")[b])
        near = filler & (H.popc(keys[:, b] ^ key) <= 1)
        keys[near, b] ^= np.uint16(0x0FF0)
        dist = H.popc(keys[:, b] ^ key)
        assert (dist == 0).sum() == length and (dist == 1).sum() == 0
    have = _check(hvd, gpu, oracle, db, 31)
    assert len(have) > length


@pytest.mark.parametrize("size", [5, 16, 17, 33])
def test_a_bucket_at_the_very_end_of_block_15(hvd, gpu, oracle, forced, size):
    """Key 0xFFFF of block 15 is the last bucket of the last block: the scalar batch of 16 words that reads its tail reads
    past the end of the words."""
    rng = np.random.default_rng(900 + size)
    first = rng.integers(0, 256, 32, dtype=np.uint8)
    first[30:32] = 255
    rows = []
    for m in range(size):
        y = first.copy()
        H.spread_over_words(rng, y, list(range(7)), (5 * m) % 36, 0)
        rows.append(y)
    db, where = _assemble(rng, rows, 2000)
    keys15 = np.ascontiguousarray(db).view("<u2")[:, 15]
    filler = np.ones(len(db), dtype=bool)
    filler[where[:size]] = False
    keys15[filler & (keys15 == 0xFFFF)] ^= np.uint16(0x0FF0)  # the bucket holds the planted rows alone
    assert (keys15 == 0xFFFF).sum() == size and keys15.max() == 0xFFFF
    have = _check(hvd, gpu, oracle, db, 31)
    assert len(have) >= size - 1
    have = _check(hvd, gpu, oracle, db, 7)
    assert len(have) >= 1
