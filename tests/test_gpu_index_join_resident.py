"""The index join as a loop (csrc/k_hamming_index.hip: k_index_join): a fixed grid whose waves each walk many work items
(block b, key u), with the survivor queue, the pair buffer and their counters carried from item to item and every queue entry
carrying its block. Index forced ("allpairs_index" 1), every DB at most 30 000 rows, pair lists equal to the CPU oracle and
every (i, j) at most once. Every case runs with 1 workgroup, with 2 and with the default grid ("index_join_wgs" 1, 2, 0).

`place` restates the kernel's map item -> (workgroup, wave, position in the wave's sequence): run = item // kRun, wave
run mod (4 x workgroups) of the grid, the runs of a wave in ascending order and inside a run the items of the rank. Before
the GPU sees a DB the tests assert with it that the planted buckets fall where the case needs them. With 1 and 2 workgroups
a wave walks all 16 blocks, so the cases are laid out for those grids; at the default grid a wave walks a few items only,
and there the same DB is simply compared with the oracle.

One case the layout cannot give: key 0x0000 (17 segments) and key 0xFFFF (no key above it) never share a wave, since their
runs are the first and the last of a block and the number of waves divides the runs of a block. The per-item-state case
therefore uses a key whose buckets above are all empty as its "no neighbour" item."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gpu_index_join_edges as E
import test_gpu_index_join_rounds as R

pytestmark = pytest.mark.gpu

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc",
                    "k_hamming_index.hip")
KRUN = int(re.search(r"constexpr uint32_t kRun = (\d+);", open(_SRC).read()).group(1))
ITEMS = 16 * 65536
RUNS = ITEMS // KRUN
GRIDS = (1, 2, 0)


def place(item, waves, world=1, rank=0):
    """(workgroup, wave of the workgroup, position in that wave's sequence) of an item of `rank`."""
    assert item % world == rank
    run = item // KRUN
    wid = run % waves
    before = np.arange(wid, run, waves, dtype=np.int64) * KRUN  # first items of the wave's earlier runs
    owned = ((before + KRUN - 1 - rank) // world - (before - 1 - rank) // world).sum()  # this rank's items inside them
    first = run * KRUN
    owned += (item - 1 - rank) // world - (first - 1 - rank) // world
    return wid // 4, wid % 4, int(owned)


def test_place_is_the_kernels_sequence():
    """The map against a literal walk: wave w of 8 takes runs w, w + 8, ..., inside a run the items of the rank."""
    for world, rank in ((1, 0), (3, 1), (7, 6)):
        for wid in (0, 5):
            seq = [i for run in range(wid, 200, 8) for i in range(run * KRUN, run * KRUN + KRUN) if i % world == rank]
            for pos, item in enumerate(seq):
                assert place(item, 8, world, rank) == (wid // 4, wid % 4, pos)


@pytest.fixture
def forced(gpu):
    E._set(gpu, b"allpairs_index", 1)
    yield
    E._set(gpu, b"allpairs_index", -1)
    E._set(gpu, b"index_join_wgs", 0)


def _waves(gpu, wgs):
    """Sets the grid; -> the waves the join's next launch has."""
    E._set(gpu, b"index_join_wgs", wgs)
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(b"index_join_wgs", C.byref(v)))
    assert v.value >= 1 and (wgs == 0 or v.value == wgs)
    return 4 * v.value


def _item(b, u):
    return b << 16 | u


def _survivors(db):
    """item -> first-stage survivors of the item: row pairs whose keys of block b are within one bit and whose word that
    holds block b is within 3 bits; the pair belongs to the item of the lower key."""
    words = np.ascontiguousarray(db).view("<u4").astype(np.uint32)
    keys = np.ascontiguousarray(db).view("<u2").astype(np.uint32)
    pop = np.unpackbits(np.arange(1 << 16, dtype="<u2").view(np.uint8).reshape(-1, 2), axis=1).sum(1)
    out = {}
    for w in range(8):
        x = words[:, w][:, None] ^ words[:, w][None, :]
        near = np.triu(pop[x & 0xFFFF] + pop[x >> 16] <= 3, 1)
        for i, j in zip(*np.nonzero(near)):
            for b in (2 * w, 2 * w + 1):
                if pop[keys[i, b] ^ keys[j, b]] <= 1:
                    it = _item(b, int(min(keys[i, b], keys[j, b])))
                    out[it] = out.get(it, 0) + 1
    return out


def _first(rng, b, u):
    row = rng.integers(0, 256, 32, dtype=np.uint8)
    E._set_key(row[None, :], [0], b, u)
    return row


def _same_word(rng, first, b):
    """A row that shares the word of block b with `first` and nothing else: a first-stage survivor, not a pair."""
    row = rng.integers(0, 256, 32, dtype=np.uint8)
    w0 = 4 * (b >> 1)
    row[w0:w0 + 4] = first[w0:w0 + 4]
    return row


def _copy_owned_by(rng, first, b, extra):
    """A near copy of `first` that block b (even) owns: two bits flipped in every lower block (no lower block qualifies) and
    `extra` bits above the word of block b."""
    assert b % 2 == 0 and 2 * b + extra <= 31
    flips = []
    for blk in range(b):
        flips += [E._bit(blk, int(t)) for t in rng.choice(16, size=2, replace=False)]
    return E._flip_bits(first, flips + E._spread(rng, list(range(b + 2, 16)), extra))


def _finish(rng, rows, clear, fillers=300):
    """planted rows + filler rows kept, in every block named in `clear` {block: keys}, more than one bit away from those
    keys (E._keep_clear's rule; with hundreds of keys a filler gets a fresh random key until it is clear); shuffled."""
    db = np.concatenate([np.array(rows), rng.integers(0, 256, (fillers, 32), dtype=np.uint8)])
    for b, keys in clear.items():
        bad = np.zeros(65536, dtype=bool)
        for u in set(keys):
            bad[[u] + [u ^ (1 << t) for t in range(16)]] = True
        for row in range(len(rows), len(db)):
            while bad[E._keys(db[row:row + 1], b)[0]]:
                E._set_key(db, [row], b, int(rng.integers(65536)))
        E._keep_clear(db, len(rows), b, [])  # (nothing left to move)
        assert not bad[E._keys(db, b)[len(rows):]].any()
    return db[rng.permutation(len(db))]


def _run_key(residue, k, j=0):
    """Key j of the k-th run of a block whose number is `residue` mod 8: in the same wave for 4 and for 8 waves."""
    return (residue + 8 * k) * KRUN + j


# ---- 1. survivors carried across items

def _carried_db():
    rng = np.random.default_rng(1)
    rows, where = [], []
    for k in range(44):
        b = (2, 6, 10, 14)[k % 4] if k < 16 else 2
        u = _run_key(1, 3 + k // 4 if k < 16 else 40 + k, k % KRUN)
        first = _first(rng, b, u)
        rows.append(first)
        rows.append(_copy_owned_by(rng, first, b, 2) if k % 3 == 0 else _same_word(rng, first, b))
        if k % 2:
            rows.append(_same_word(rng, first, b))  # three rows: three survivors
        where.append((b, u))
    clear = {}
    for b, u in where:
        clear.setdefault(b, []).extend([u] + [u ^ (1 << t) for t in range(16)])
    return _finish(rng, rows, clear), where


@pytest.mark.parametrize("wgs", GRIDS)
def test_survivors_carried_across_items(hvd, gpu, oracle, forced, wgs):
    db, where = _carried_db()
    waves = _waves(gpu, wgs)
    surv = _survivors(db)
    if wgs:
        spots = sorted(place(_item(b, u), waves) + (surv[_item(b, u)],) for b, u in where)
        assert len({s[:2] for s in spots}) == 1  # one wave walks them all
        assert all(1 <= s[3] <= 5 for s in spots)
        total = np.cumsum([s[3] for s in spots])
        assert total[-1] >= 64 and total[0] < 64  # the 64th pending survivor arrives in a later item than the first
        assert len({b for b, _ in where}) == 4  # ... and the queue then holds entries of several blocks
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) >= 14


# ---- 2. survivors pending across a block change: a drain with the wrong block would change their verdict

def _block_change_db():
    """Block 4, key 0xFFFF -- the last item a wave walks in block 4 -- holds three near copies that block 4 owns (drained as
    block 8 they would be dropped: blocks 4 and 5 lie below). The wave's later bucket in block 8 holds near copies that
    block 6 owns (drained as block 4 they would come out a second time: nothing below block 4 qualifies)."""
    rng = np.random.default_rng(2)
    u4, u8 = 0xFFFF, _run_key((0x10000 // KRUN - 1) % 8, 5)
    a = _first(rng, 4, u4)
    rows = [a, _copy_owned_by(rng, a, 4, 3), _copy_owned_by(rng, a, 4, 5)]
    c = _first(rng, 8, u8)
    for _ in range(2):  # two bits in each of the blocks 0..5, none in 6..9, a few above: block 6 is the first that qualifies
        flips = []
        for blk in range(6):
            flips += [E._bit(blk, int(t)) for t in rng.choice(16, size=2, replace=False)]
        rows.append(E._flip_bits(c, flips + E._spread(rng, list(range(10, 16)), 2)))
    rows.append(c)
    clear = {4: [u4] + [u4 ^ (1 << t) for t in range(16)], 8: [u8] + [u8 ^ (1 << t) for t in range(16)]}
    return _finish(rng, rows, clear, fillers=200), u4, u8


@pytest.mark.parametrize("wgs", GRIDS)
def test_survivors_pending_across_a_block_change(hvd, gpu, oracle, forced, wgs):
    db, u4, u8 = _block_change_db()
    waves = _waves(gpu, wgs)
    surv = _survivors(db)
    assert surv[_item(4, u4)] == 3 and surv[_item(8, u8)] == 3
    if wgs:
        p4, p8 = place(_item(4, u4), waves), place(_item(8, u8), waves)
        assert p4[:2] == p8[:2] and p4[2] < p8[2]
        # nothing of the wave's sequence lies behind key 0xFFFF in block 4: its next item is in another block
        assert all(place(it, waves)[:2] != p4[:2] or not (4 << 16 | u4) < it < (5 << 16) for it in surv)
        # fewer than 64 survivors in the whole wave: nothing is drained before its end, the one drain mixes the blocks
        mine = [n for it, n in surv.items() if place(it, waves)[:2] == p4[:2]]
        assert 6 <= sum(mine) < 64
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) == 6  # three pairs among the rows of block 4's bucket, three among block 8's (owned by block 6)


# ---- 3. the pair buffer across items, and the overflow contract

def _pair_buffer_db():
    rng = np.random.default_rng(3)
    rows, keys = [], []
    k = -1
    while len(keys) < 70:
        k += 1
        u = _run_key(2, k)
        if any(bin(u ^ v).count("1") < 2 for v in keys):
            continue  # (planted keys are not each other's neighbours: an item's survivors are its bucket's alone)
        first = _first(rng, 0, u)
        rows += [first, _copy_owned_by(rng, first, 0, 5), _copy_owned_by(rng, first, 0, 9)]
        keys.append(u)
    clear = {0: [v for u in keys for v in [u] + [u ^ (1 << t) for t in range(16)]]}
    return _finish(rng, rows, clear), keys


@pytest.mark.parametrize("wgs", GRIDS)
def test_pair_buffer_across_items_and_overflow(hvd, gpu, oracle, forced, wgs):
    db, keys = _pair_buffer_db()
    waves = _waves(gpu, wgs)
    surv = _survivors(db)
    if wgs:
        spots = sorted(place(_item(0, u), waves) for u in keys)
        assert len({s[:2] for s in spots}) == 1
        assert all(surv[_item(0, u)] == 3 for u in keys)
        # 210 pairs, 3 to an item: drains of 64 at the 22nd, 43rd and 64th bucket, the second of them finds the buffer
        # full and flushes it in the middle of the sequence; the rest leaves at the wave's end
        assert 3 * len(keys) > 3 * 64
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) >= 210
    cap = 100
    out = np.zeros(cap, dtype=want.dtype)
    cnt = C.c_int64(0)
    rc = gpu.load().hvd_allpairs_hamming256(db.ctypes.data, len(db), None, 31, out.ctypes.data, cap, C.byref(cnt))
    assert rc == gpu.HVD_ERR_OVERFLOW and cnt.value == len(want)


# ---- 4. per-item state: y lists of different structure in consecutive items of one wave

def _structures_db():
    b = 5
    parts = [
        (0x0000, 3, {t: 1 + t % 3 for t in range(16)}),  # 17 segments in one round
        (_run_key(0, 31, 0) | 0x0300, 4, {}),  # every bucket above it is empty: the y list is the bucket alone
        (0xE000, 10, {1: 1, 2: 16, 3: 17, 5: 170, 8: 1, 9: 16, 12: 17}),  # a segment over three rounds; key 0xE001 stays empty
        (0xF0C0, 65, {1: 5, 11: 30}),  # a bucket of 65
    ]
    rng = np.random.default_rng(4)
    dbs, keys = [], []
    for k, (u, own, sizes) in enumerate(parts):
        assert (u // KRUN) % 8 == 0 and all(not (u >> t) & 1 for t in sizes)
        dbs.append(R._segments_db(b, u, own, sizes, seed=600 + k, fillers=0))
        keys += [u] + [u ^ (1 << t) for t in range(16)]
    planted = np.concatenate(dbs)
    db = np.concatenate([planted, rng.integers(0, 256, (400, 32), dtype=np.uint8)])
    E._keep_clear(db, len(planted), b, sorted(set(keys)))
    return db[rng.permutation(len(db))], b, parts


@pytest.mark.parametrize("wgs", GRIDS)
def test_per_item_state_over_different_y_lists(hvd, gpu, oracle, forced, wgs):
    db, b, parts = _structures_db()
    waves = _waves(gpu, wgs)
    for u, own, sizes in parts:
        assert R._ylist(db, b, u) == [own] + [sizes.get(t, 0) for t in range(16)]
    assert all(s >= 1 for s in R._ylist(db, b, 0x0000)) and sum(R._ylist(db, b, 0x0000)) <= 64
    assert R._ylist(db, b, parts[1][0])[1:] == [0] * 16 and bin(parts[1][0]).count("1") < 16
    assert R._ylist(db, b, 0xE001)[0] == 0  # the empty bucket between them
    first = 10 + 34
    assert (first + 170 - 1) // 64 - first // 64 >= 2
    if wgs:
        spots = [place(_item(b, u), waves) for u, _, _ in parts] + [place(_item(b, 0xE001), waves)]
        assert len({s[:2] for s in spots}) == 1
        order = [s[2] for s in spots]
        assert order[0] < order[1] < order[2] < order[4] < order[3]  # 17 segments, bucket alone, three rounds, empty, 65
    R._check(hvd, gpu, oracle, db)


# ---- 5. the ends of the item space, grids that do not divide the runs, more waves than runs

def _ends_db():
    rng = np.random.default_rng(5)
    rows = []
    a = _first(rng, 0, 0x0000)
    rows += [a, _copy_owned_by(rng, a, 0, 7), _copy_owned_by(rng, a, 0, 11)]
    z = _first(rng, 15, 0xFFFF)
    for extra in (0, 1):  # block 15 owns a pair only if no block below it qualifies: two bits in each of the blocks 0..13
        flips = []
        for blk in range(14):
            flips += [E._bit(blk, int(t)) for t in rng.choice(16, size=2, replace=False)]
        rows.append(E._flip_bits(z, flips + ([E._bit(14, 3)] if extra else [])))
    rows.append(z)
    db = np.concatenate([np.array(rows), rng.integers(0, 256, (500, 32), dtype=np.uint8)])
    for k in range(10, 200, 4):  # and pairs anywhere
        db[k + 1] = E._flip_outside(rng, db[k], (3 * k) % 36, set())
    return db[rng.permutation(len(db))]


@pytest.mark.parametrize("wgs", GRIDS + (3, 5, RUNS // 4 + 7))
def test_ends_of_the_item_space_and_odd_grids(hvd, gpu, oracle, forced, wgs):
    db = _ends_db()
    waves = _waves(gpu, wgs)
    counts0, counts15 = np.bincount(E._keys(db, 0), minlength=65536), np.bincount(E._keys(db, 15), minlength=65536)
    assert counts0[0x0000] >= 3 and counts15[0xFFFF] >= 3
    assert place(_item(0, 0), waves)[2] == 0  # the first item of wave 0
    last = place(_item(15, 0xFFFF), waves)
    assert last[0] * 4 + last[1] == (RUNS - 1) % waves
    if wgs in (3, 5):
        assert RUNS % waves != 0
    if wgs > RUNS // 4:
        assert waves > RUNS  # the waves from RUNS on walk nothing
    want = R._check(hvd, gpu, oracle, db)
    have = set(zip(want["i"].tolist(), want["j"].tolist()))
    assert len(have) >= 6 + 20


# ---- 6. ranks: the items of a run belong to different ranks

def _rank_db():
    rng = np.random.default_rng(6)
    rows = []
    for k in range(40):
        b = 2 * (k % 8)
        u = _run_key(k % 8, 10 + k, 0)  # an even key: u ^ 1 is the next item, of another rank
        first = _first(rng, b, u)
        twin = _copy_owned_by(rng, first, b, 3)
        other = E._flip_bits(_copy_owned_by(rng, first, b, 1), [E._bit(b, 0)])  # in bucket u ^ 1, a pair with `first`
        rows += [first, twin, other]
        assert int(E._keys(other[None, :], b)[0]) == u ^ 1 and u // KRUN == (u ^ 1) // KRUN  # the same run, the next item
    db = np.concatenate([np.array(rows), rng.integers(0, 256, (600, 32), dtype=np.uint8)])
    for k in range(130, 500, 3):
        db[k + 1] = E._flip_outside(rng, db[k], (5 * k) % 38, set())
    return db[rng.permutation(len(db))]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("wgs", GRIDS)
def test_ranks_share_the_items_of_a_run(hvd, gpu, oracle, forced, wgs, world):
    from hvd_amd import multigpu

    db = _rank_db()
    _waves(gpu, wgs)
    assert all(_item(b, 0) % world != _item(b, 1) % world for b in range(16))  # keys u and u ^ 1: items of different ranks
    want = oracle.allpairs(db, 31)
    lib = gpu.load()
    d_db = gpu.DeviceBuffer.from_array(db)
    d_img = multigpu.expand_fp4(d_db.ptr, len(db))
    cap = 4 * len(want) + 64
    d_pairs, d_cnt = gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)
    lists = []
    for rank in range(world):
        d_cnt.zero()
        gpu.check(lib.hvd_dev_allpairs_hamming256_mfma(d_db.ptr, d_img.ptr, len(db), None, 31, rank, world, d_pairs.ptr, cap,
                                                       d_cnt.ptr, 13))
        found = int(d_cnt.to_array(np.uint64, 1)[0])  # (the copy waits for the stream)
        v = C.c_int(0)
        gpu.check(lib.hvd_debug_get(b"allpairs_index_used", C.byref(v)))
        assert v.value == 1 and found <= cap
        lists.append(d_pairs.to_array(want.dtype, found))
    for d in (d_db, d_img, d_pairs, d_cnt):
        d.free()
    got = np.concatenate(lists)
    assert len(np.unique(got[["i", "j"]])) == len(got)  # the rank lists are disjoint
    assert all(len(part) > 0 for part in lists)
    assert np.array_equal(np.sort(got, order=["i", "j"]), want), (len(got), len(want))
    assert len(want) >= 3 * 40
