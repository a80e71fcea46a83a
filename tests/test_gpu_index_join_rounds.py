"""Rounds, segments and drains of the index join (csrc/k_hamming_index.hip: k_index_join) with the index forced
("allpairs_index" 1), pair lists equal to the CPU oracle and every (i, j) at most once. The y list of a work item (block b,
key u) is its bucket followed by the buckets of the one-bit neighbours above u, walked 64 entries to a round by a cursor
over the segments: all 17 segments inside one round and the key with no neighbour above it, empty segments first, in the
middle and last, segments that end exactly on a round, one segment over several rounds between short ones, a bucket of 64
and 65 (the i < j limit on a round boundary). The full check evaluates the ownership rule only when some lane of the drain
is within max_dist: a bucket whose drains emit nothing next to pairs at distances 0, 31 and 32, and a bucket whose drains
mix pairs block b owns, pairs a lower block owns, pairs a lower block only seems to own, pairs beyond 31 and pairs a group
array removes. Every DB's bucket layout is asserted with numpy before the GPU sees it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_index_join_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture
def forced(gpu):
    E._set(gpu, b"allpairs_index", 1)
    yield
    E._set(gpu, b"allpairs_index", -1)


def _check(hvd, gpu, oracle, db, group=None):
    assert len(db) <= 30000
    want = oracle.allpairs(db, 31, group=group)
    got = hvd.allpairs_hamming(db, 31, group=group)
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(b"allpairs_index_used", C.byref(v)))
    assert v.value == 1
    assert len(np.unique(got[["i", "j"]])) == len(got)
    assert np.array_equal(got, want), (len(got), len(want))
    return want


def _ylist(db, b, u):
    """Sizes of the 17 segments of work item (b, u) in the y list's order: the bucket, then neighbour t = 0 .. 15 (0 where
    u ^ (1 << t) lies below u: not in the list)."""
    counts = np.bincount(E._keys(db, b), minlength=65536)
    return [int(counts[u])] + [0 if (u >> t) & 1 else int(counts[u ^ (1 << t)]) for t in range(16)]


def _segments_db(b, u, own, sizes, seed, fillers=400):
    """Key u of block b: `own` rows in the bucket and sizes[t] rows in the bucket u ^ (1 << t), every one of them a bucket
    member with that key bit and a few bits outside block b flipped (near-duplicates inside the bucket and between it and
    every segment), then filler rows whose keys of block b stay two bits away from u and from all its neighbours."""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, 256, 32, dtype=np.uint8)
    E._set_key(first[None, :], [0], b, u)
    members = [E._flip_outside(rng, first, (3 * m) % 14, {b}) for m in range(own)]
    rows = list(members)
    for t in sorted(sizes):
        for m in range(sizes[t]):
            row = E._flip_outside(rng, members[m % own], (5 * m) % 34, {b})
            rows.append(E._flip_bits(row, [E._bit(b, t)]))
    planted = len(rows)
    db = np.concatenate([np.array(rows), rng.integers(0, 256, (fillers, 32), dtype=np.uint8)])
    E._keep_clear(db, planted, b, [u] + [u ^ (1 << t) for t in range(16)])
    counts = np.bincount(E._keys(db, b), minlength=65536)
    assert int(counts[u]) == own and all(int(counts[u ^ (1 << t)]) == sizes.get(t, 0) for t in range(16))
    return db[rng.permutation(len(db))]


# ---- 1. every neighbour segment inside one round; the key with no neighbour above it

@pytest.mark.parametrize("b", [0, 15])
def test_all_seventeen_segments_in_one_round(hvd, gpu, oracle, forced, b):
    sizes = {t: 1 + t % 3 for t in range(16)}
    db = _segments_db(b, 0x0000, 3, sizes, seed=100 + b)
    seg = _ylist(db, b, 0x0000)
    assert seg == [3] + [sizes[t] for t in range(16)] and all(s >= 1 for s in seg) and sum(seg) <= 64
    want = _check(hvd, gpu, oracle, db)
    assert len(want) >= sum(seg) - 3


@pytest.mark.parametrize("b", [0, 15])
def test_the_key_with_no_neighbour_above(hvd, gpu, oracle, forced, b):
    sizes = {t: 1 + t % 3 for t in range(16)}
    db = _segments_db(b, 0xFFFF, 3, sizes, seed=110 + b)
    assert _ylist(db, b, 0xFFFF) == [3] + [0] * 16  # the y list is the bucket alone
    for t in range(16):  # ... and every neighbour below sees it as its only neighbour: 16 - t empty segments, then t more
        seg = _ylist(db, b, 0xFFFF ^ (1 << t))
        assert seg == [sizes[t]] + [0] * t + [3] + [0] * (15 - t)
    want = _check(hvd, gpu, oracle, db)
    assert len(want) >= sum(sizes.values())


# ---- 2. empty segments first, in the middle and last

@pytest.mark.parametrize("name,own,sizes", [
    ("first_middle_last", 5, {4: 3, 5: 20, 10: 40, 11: 2}),  # t = 0..3, 6..9 and 12..15 empty; 70 entries: two rounds
    ("only_the_last_neighbour", 5, {15: 70}),
    ("only_the_last_neighbour_one_round", 5, {15: 7}),
    ("every_other_one", 4, {t: 9 for t in range(0, 16, 2)}),
    ("first_and_last", 2, {0: 1, 15: 1}),
])
def test_empty_segments(hvd, gpu, oracle, forced, name, own, sizes):
    b = 6 if len(sizes) % 2 else 9
    db = _segments_db(b, 0x0000, own, sizes, seed=200 + len(name))
    seg = _ylist(db, b, 0x0000)
    assert seg == [own] + [sizes.get(t, 0) for t in range(16)]
    assert seg.count(0) == 16 - len(sizes)
    if name == "first_middle_last":
        assert seg[1:5] == [0] * 4 and seg[7:11] == [0] * 4 and seg[13:] == [0] * 4 and sum(seg) > 64
    want = _check(hvd, gpu, oracle, db)
    assert len(want) >= sum(sizes.values())


# ---- 3. round boundaries against segment boundaries

def test_segments_that_end_exactly_on_a_round(hvd, gpu, oracle, forced):
    own, sizes = 20, {0: 44, 3: 64, 7: 10}
    db = _segments_db(4, 0x0000, own, sizes, seed=300)
    ends = np.cumsum([s for s in _ylist(db, 4, 0x0000) if s]).tolist()
    assert ends == [20, 64, 128, 138]
    _check(hvd, gpu, oracle, db)


@pytest.mark.parametrize("own,long", [(30, 170), (10, 170), (30, 200), (13, 150)])
def test_one_segment_over_several_rounds_between_short_ones(hvd, gpu, oracle, forced, own, long):
    sizes = {1: 1, 2: 16, 3: 17, 5: long, 8: 1, 9: 16, 12: 17}
    db = _segments_db(11, 0x0000, own, sizes, seed=310 + own + long)
    seg = _ylist(db, 11, 0x0000)
    assert [s for s in seg if s] == [own, 1, 16, 17, long, 1, 16, 17]
    first = own + 34  # the long segment's first entry and its last: at least three rounds
    last = first + long - 1
    assert last // 64 - first // 64 >= 2
    if own == 30:
        assert first % 64 == 0  # it begins on a round, behind three short segments
    _check(hvd, gpu, oracle, db)


@pytest.mark.parametrize("own", [64, 65])
def test_own_bucket_ends_on_a_round(hvd, gpu, oracle, forced, own):
    sizes = {2: 5, 13: 30}
    db = _segments_db(1, 0x0000, own, sizes, seed=320 + own)
    assert [s for s in _ylist(db, 1, 0x0000) if s] == [own, 5, 30]
    want = _check(hvd, gpu, oracle, db)
    assert len(want) >= own * (own - 1) // 4


# ---- 4. drains that emit nothing, then some that do

def _pairwise(rows):
    bits = np.unpackbits(rows, axis=1).astype(np.int32)
    return bits @ (1 - bits).T + (1 - bits) @ bits.T


@pytest.mark.parametrize("b", [3, 12])
def test_drains_that_emit_nothing_next_to_pairs_at_the_boundary(hvd, gpu, oracle, forced, b):
    rng = np.random.default_rng(400 + b)
    word = rng.integers(0, 256, 4, dtype=np.uint8)
    w0 = 4 * (b >> 1)  # the bytes of the word that holds block b
    crowd = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    crowd[:, w0:w0 + 4] = word
    d = _pairwise(crowd)
    iu = np.triu_indices(200, 1)
    assert d[iu].min() > 31  # every pair passes the word test (the word is shared), none is within max_dist
    survivors = int((_pairwise(np.ascontiguousarray(crowd[:, w0:w0 + 4]))[iu] <= 3).sum())
    assert survivors == 200 * 199 // 2 >= 64
    rows, expect = [crowd], 0
    for k in (0, 31, 32, 0, 31, 32):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        a[w0:w0 + 4] = word
        rows.append(np.stack([a, E._flip_outside(rng, a, k, {b, b ^ 1})]))
        expect += k <= 31
    planted = np.concatenate(rows)
    db = np.concatenate([planted, rng.integers(0, 256, (500, 32), dtype=np.uint8)])
    u = int(E._keys(planted[:1], b)[0])
    E._keep_clear(db, len(planted), b, [u] + [u ^ (1 << t) for t in range(16)])
    assert int((E._keys(db, b) == u).sum()) == 212
    db = db[rng.permutation(len(db))]
    want = _check(hvd, gpu, oracle, db)
    assert len(want) == expect == 4 and sorted(want["dist"].tolist()) == [0, 0, 31, 31]


# ---- 5. one bucket whose drains mix every kind of lane

def _qualifying(x, y):
    """Blocks that qualify for the pair at max_dist 31: keys within r = 1 and the word that holds the block within tw = 3."""
    dx = np.unpackbits(x ^ y)
    return [blk for blk in range(16)
            if dx[16 * blk:16 * blk + 16].sum() <= 1 and dx[32 * (blk >> 1):32 * (blk >> 1) + 32].sum() <= 3]


def _flips(rng, per_block):
    out = []
    for blk, cnt in per_block.items():
        out += [E._bit(blk, int(t)) for t in rng.choice(16, size=cnt, replace=False)]
    return out


@pytest.mark.parametrize("b", [6, 10])
def test_mixed_lanes_in_one_drain(hvd, gpu, oracle, forced, b):
    """All planted rows share the whole word of block b (b even: its sibling lies above it), so every pair among them
    survives the first stage and the pairs share drains. kind -> bits flipped per lower block, then `extra` bits above the
    word: own (two bits in every lower block: block b is the first that qualifies), lower (block 2 has one bit and its word
    three: it qualifies and owns the pair), lower_odd (block 3 untouched, its word two), seems (block 2 has one bit, but
    its word four: beyond tw, block b owns the pair)."""
    rng = np.random.default_rng(500 + b)
    low = {blk: 2 for blk in range(b)}
    kinds = {"own": low, "lower": {**low, 2: 1, 3: 2}, "lower_odd": {**low, 2: 2, 3: 0}, "seems": {**low, 2: 1, 3: 3}}
    above = list(range(b + 2, 16))
    word = rng.integers(0, 256, 4, dtype=np.uint8)
    w0 = 4 * (b >> 1)
    rows, plan = [], []
    for rep in range(12):
        for kind, per in kinds.items():
            base = sum(per.values())
            for total in (base, 31, 32):
                a = rng.integers(0, 256, 32, dtype=np.uint8)
                a[w0:w0 + 4] = word
                partner = E._flip_bits(a, _flips(rng, per) + E._spread(rng, above, total - base))
                q = _qualifying(a, partner)
                assert int(np.unpackbits(a ^ partner).sum()) == total and b in q
                assert min(q) == {"own": b, "lower": 2, "lower_odd": 3, "seems": b}[kind], (kind, q)
                plan.append((len(rows), len(rows) + 1, kind, total))
                rows += [a, partner]
    planted = np.array(rows)
    db = np.concatenate([planted, rng.integers(0, 256, (500, 32), dtype=np.uint8)])
    u = int(E._keys(planted[:1], b)[0])
    E._keep_clear(db, len(planted), b, [u] + [u ^ (1 << t) for t in range(16)])
    assert int((E._keys(db, b) == u).sum()) == len(planted) == 288  # one bucket of block b holds them all
    group = np.arange(len(db), dtype=np.int32)
    removed = [(i, j) for i, j, kind, total in plan if kind == "own" and total <= 31][::3]
    for i, j in removed:
        group[j] = group[i]
    perm = rng.permutation(len(db))
    inv = np.argsort(perm)
    db, group = db[perm], group[perm]
    for g in (None, group):
        want = _check(hvd, gpu, oracle, db, group=g)
        have = set(zip(want["i"].tolist(), want["j"].tolist()))
        for i, j, kind, total in plan:
            pi, pj = sorted((int(inv[i]), int(inv[j])))
            assert ((pi, pj) in have) == (total <= 31 and not (g is not None and (i, j) in removed)), (kind, total)
