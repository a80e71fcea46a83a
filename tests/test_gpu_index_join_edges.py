"""Edges of the index join (csrc/k_hamming_index.hip: k_index_join on the half-width index) with the index forced
("allpairs_index" 1), pair lists equal to the CPU oracle: bucket sizes around the scalar x batch and around 64 in the first
and last block of either half, y lists that end just before, at and just after a round of 64, pairs whose differing bits lie
only in the half the index stores, only in the half the survivors fetch from the packed DB, or in both, pairs within r in
two blocks with a group array, and enough pairs from one bucket that the waves' pair buffers flush many times. Every DB's
structure is asserted with numpy before the GPU sees it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)


def _set(gpu, key, value):
    gpu.check(gpu.load().hvd_debug_set(key, value))


def _used(gpu):
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(b"allpairs_index_used", C.byref(v)))
    return v.value


@pytest.fixture
def forced(gpu):
    _set(gpu, b"allpairs_index", 1)
    yield
    _set(gpu, b"allpairs_index", -1)


def _keys(db, b):
    """Key of block b of every hash: bits 16b..16b+15 of the packed hash = the b-th little-endian 16-bit word."""
    return np.ascontiguousarray(db).view("<u2")[:, b].astype(np.uint32)


def _set_key(db, rows, b, key):
    db[rows, 2 * b] = key & 255
    db[rows, 2 * b + 1] = key >> 8


def _popc16(x):
    return np.unpackbits(np.asarray(x, dtype="<u2").view(np.uint8).reshape(-1, 2), axis=1).sum(1)


def _bit(b, t):
    """Index into np.unpackbits(hash) of bit t of block b (np.unpackbits is MSB first inside a byte)."""
    return (2 * b + t // 8) * 8 + (7 - t % 8)


def _flip_bits(row, positions):
    bits = np.unpackbits(row.copy())
    bits[np.asarray(positions, dtype=np.int64)] ^= 1
    return np.packbits(bits)


def _flip_outside(rng, row, k, blocks):
    """row with k bits flipped, none of them in `blocks`."""
    free = [_bit(b, t) for b in range(16) if b not in blocks for t in range(16)]
    return _flip_bits(row, rng.choice(free, size=k, replace=False))


def _keep_clear(db, first_filler, b, keys):
    """Filler rows (first_filler ..) whose key of block b is within one bit of any of `keys` get another key."""
    for _ in range(4):
        kb = _keys(db, b)[first_filler:]
        near = np.zeros(len(kb), dtype=bool)
        for u in keys:
            near |= _popc16(kb ^ u) <= 1
        if not near.any():
            return
        rows = first_filler + np.flatnonzero(near)
        _set_key(db, rows, b, (kb[near] ^ 0x0FF0) & 0xFFFF)
    raise AssertionError("filler keys still near a planted key")


def _half_dist(x, y, half):
    return int(np.unpackbits(x[16 * half:16 * half + 16] ^ y[16 * half:16 * half + 16]).sum())


def _check(hvd, gpu, oracle, db, md=31, group=None):
    want = oracle.allpairs(db, md, group=group)
    got = hvd.allpairs_hamming(db, md, group=group)
    assert _used(gpu) == 1
    assert np.array_equal(got, want), (len(got), len(want))
    return want


def _bucket_db(b, seed):
    """One bucket of block b per size in SIZES (keys pairwise >= 3 bits apart), members = one row with 0..40 bits flipped
    outside block b, and 600 filler rows whose keys of block b stay away from those buckets."""
    rng = np.random.default_rng(seed)
    keys = [0x0007 * (i + 1) ^ (0x1000 * (i + 1)) for i in range(len(SIZES))]
    rows = []
    for size, u in zip(SIZES, keys):
        first = rng.integers(0, 256, 32, dtype=np.uint8)
        _set_key(first[None, :], [0], b, u)
        rows += [_flip_outside(rng, first, (7 * m) % 41, {b}) for m in range(size)]
    planted = len(rows)
    db = np.concatenate([np.array(rows), rng.integers(0, 256, (600, 32), dtype=np.uint8)])
    _keep_clear(db, planted, b, keys)
    perm = rng.permutation(len(db))
    return db[perm], keys


@pytest.mark.parametrize("b", [0, 7, 8, 15])
def test_bucket_sizes_around_the_batch_and_around_64(hvd, gpu, oracle, forced, b):
    db, keys = _bucket_db(b, seed=40 + b)
    assert len(db) <= 5000
    kb = _keys(db, b)
    for i, u in enumerate(keys):
        for w in keys[i + 1:]:
            assert bin(u ^ w).count("1") >= 3
    counts = np.bincount(kb, minlength=65536)
    assert [int(counts[u]) for u in keys] == list(SIZES)
    for u in keys:  # nothing but the bucket itself in its y list
        assert sum(int(counts[u ^ (1 << t)]) for t in range(16)) == 0
    want = _check(hvd, gpu, oracle, db)
    assert len(want) > 100


def _ylist_db(length, b, seed):
    """Key u = 0x0100 of block b: 20 rows in the bucket, and length - 20 rows in the one-bit neighbours above u (bits 0, 5
    and 15, in the y list's order), every one of them a bucket member with its key bit and a few other bits flipped -- so
    near-duplicates lie inside the bucket and between it and every round of the y list."""
    rng = np.random.default_rng(seed)
    u, own = 0x0100, 20
    rest = length - own
    sizes = {0: rest // 3, 5: rest // 3, 15: rest - 2 * (rest // 3)}
    first = rng.integers(0, 256, 32, dtype=np.uint8)
    _set_key(first[None, :], [0], b, u)
    members = [_flip_outside(rng, first, (3 * m) % 14, {b}) for m in range(own)]
    rows = list(members)
    for t, size in sizes.items():
        for m in range(size):
            row = _flip_outside(rng, members[m % own], (5 * m) % 34, {b})
            rows.append(_flip_bits(row, [_bit(b, t)]))
    planted = len(rows)
    db = np.concatenate([np.array(rows), rng.integers(0, 256, (500, 32), dtype=np.uint8)])
    _keep_clear(db, planted, b, [u])
    perm = rng.permutation(len(db))
    return db[perm], u, sizes


@pytest.mark.parametrize("length", [63, 64, 65, 127, 128, 129])
def test_y_lists_that_end_around_a_round(hvd, gpu, oracle, forced, length):
    b = 5 if length % 2 else 10
    db, u, sizes = _ylist_db(length, b, seed=length)
    assert len(db) <= 5000
    counts = np.bincount(_keys(db, b), minlength=65536)
    assert counts[u] == 20
    above = [u ^ (1 << t) for t in range(16) if not (u >> t) & 1]
    assert all(v > u for v in above) and len(above) == 15
    assert int(counts[u]) + sum(int(counts[v]) for v in above) == length
    # the y list in its order: the bucket, then the neighbours by ascending bit -- where each neighbour's entries fall
    ends = np.cumsum([20] + [int(counts[u ^ (1 << t)]) for t in range(16) if not (u >> t) & 1])
    assert ends[-1] == length and [int(counts[u ^ (1 << t)]) for t in (0, 5, 15)] == [sizes[0], sizes[5], sizes[15]]
    if length > 64:
        assert (ends[-1] - 1) // 64 >= 1  # the last neighbour reaches the second round
    if length > 128:
        assert (ends[-1] - 1) // 64 == 2  # ... and the third
    want = _check(hvd, gpu, oracle, db)
    assert len(want) >= length - 20


def _spread(rng, blocks, k, base=0):
    """k bit positions spread evenly over `blocks` (at least 2 per block when k >= 2 len(blocks)), beginning at block `base`."""
    out = []
    per = [k // len(blocks) + (1 if i < k % len(blocks) else 0) for i in range(len(blocks))]
    for blk, cnt in zip(blocks, per):
        out += [_bit(blk, int(t)) for t in rng.choice(16, size=cnt, replace=False)]
    return out


@pytest.mark.parametrize("b", [0, 7, 8, 15])
def test_distance_splits_between_the_indexed_and_the_fetched_half(hvd, gpu, oracle, forced, b):
    """Pairs that share the key of block b. `hold` = the half that holds block b (fetched from the packed DB by block b's
    work item), `other` = the half its index stores. Differing bits (hold, other): (31, 0) and (32, 0) -- the first stage
    sees distance 0, the fetched half decides; (0, 31) and (0, 32); (1, 31) and (1, 30)."""
    rng = np.random.default_rng(70 + b)
    hold = 0 if b < 8 else 1
    hold_blocks = [x for x in range(8 * hold, 8 * hold + 8) if x != b]
    other_blocks = list(range(8 * (1 - hold), 8 * (1 - hold) + 8))
    splits = [(31, 0, True), (32, 0, False), (0, 31, True), (0, 32, False), (1, 31, False), (1, 30, True)]
    db = rng.integers(0, 256, (1200, 32), dtype=np.uint8)
    expect = []
    for k in range(0, 600, 2):
        in_hold, in_other, accept = splits[(k // 2) % len(splits)]
        db[k + 1] = _flip_bits(db[k], _spread(rng, hold_blocks, in_hold) + _spread(rng, other_blocks, in_other))
        assert _keys(db[k:k + 2], b)[0] == _keys(db[k:k + 2], b)[1]
        assert _half_dist(db[k], db[k + 1], hold) == in_hold and _half_dist(db[k], db[k + 1], 1 - hold) == in_other
        expect.append((k, k + 1, accept))
    want = _check(hvd, gpu, oracle, db)
    have = set(zip(want["i"].tolist(), want["j"].tolist()))
    for i, j, accept in expect:
        assert ((i, j) in have) == accept, (i, j, accept)


def test_pairs_within_r_in_two_blocks_come_out_once_and_groups_remove_some(hvd, gpu, oracle, forced):
    rng = np.random.default_rng(9)
    db = rng.integers(0, 256, (1500, 32), dtype=np.uint8)
    claimed = []
    for k in range(0, 800, 2):
        b1, b2 = sorted(int(x) for x in rng.choice(16, size=2, replace=False))
        flips = []
        for blk in range(16):  # two bits in every other block (28), none or one in the two blocks that claim the pair
            cnt = int(rng.integers(0, 2)) if blk in (b1, b2) else 2
            flips += [_bit(blk, int(t)) for t in rng.choice(16, size=cnt, replace=False)]
        db[k + 1] = _flip_bits(db[k], flips)
        within = [blk for blk in range(16) if _popc16(_keys(db[k:k + 1], blk) ^ _keys(db[k + 1:k + 2], blk))[0] <= 1]
        assert within == [b1, b2]
        claimed.append((k, k + 1))
    group = np.arange(len(db), dtype=np.int32)
    group[1:800:6] = group[0:800:6]  # every third planted pair shares a group: removed
    same = sum(1 for i, j in claimed if group[i] == group[j])
    assert 100 < same < len(claimed)
    want = _check(hvd, gpu, oracle, db, group=group)
    have = set(zip(want["i"].tolist(), want["j"].tolist()))
    for i, j in claimed:
        assert ((i, j) in have) == (group[i] != group[j])
    _check(hvd, gpu, oracle, db)  # and without the groups: every one of them, once


def test_one_bucket_of_identical_rows_flushes_the_pair_buffer_many_times(hvd, gpu, oracle, forced):
    rng = np.random.default_rng(11)
    db = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    rows = rng.choice(1000, size=200, replace=False)
    db[rows] = db[rows[0]]
    assert len(np.unique(db, axis=0)) == 801
    want = _check(hvd, gpu, oracle, db)
    assert len(want) == 19900
