"""Consecutive work items of one wave of the index join (csrc/k_hamming_index.hip: k_index_join): what a wave carries from
an item to the next one, or fetches for the next one while it walks the current one, must be the right item's. Index forced
("allpairs_index" 1), every DB at most 30 000 rows, every pair list equal to the CPU oracle's brute force with every (i, j)
at most once, every case with 1 workgroup, with 2 and with the default grid ("index_join_wgs" 1, 2, 0).

S is the number of y entries an item may have fetched ahead: `constexpr uint32_t kStage = N;` of the source where the kernel
has one, else 128 -- two rounds of 64, the size DESIGN 4.1 measured and did not keep -- so the lengths below stay on and
around the round boundaries either way. At these sizes almost every item is empty, so the cases plant their buckets: `place`
(test_gpu_index_join_resident) restates the kernel's map item -> (workgroup, wave, position), and every layout is asserted
with it and with numpy before the GPU sees the DB. The layouts are built for the number of waves of the grid (4 or 8); the
default grid gets the layout for 8 and is simply compared with the oracle.

A y list of length 1 is a bucket of one row with nothing above it, so its key cannot have the other keys of its run above
it non-empty: where the case asks for all four keys of a run, the length 1 sits on the run's last key (it has no neighbour
inside the run), and as a wave's FIRST non-empty item it sits on the last key of a run that holds nothing else."""
import ctypes as C
import re

import numpy as np
import pytest

import test_gpu_index_join_edges as E
import test_gpu_index_join_resident as T
import test_gpu_index_join_rounds as R

pytestmark = pytest.mark.gpu

_m = re.search(r"constexpr uint32_t kStage = (\d+);", open(T._SRC).read())
S = int(_m.group(1)) if _m else 128
assert S % 64 == 0 and S >= 64
KRUN = T.KRUN
RUNS_PER_BLOCK = 65536 // KRUN
GRIDS = (1, 2, 0)
LENGTHS = (1, S - 1, S, S + 1, S + 63, S + 64, S + 65, 3 * S)


@pytest.fixture
def forced(gpu):
    E._set(gpu, b"allpairs_index", 1)
    yield
    E._set(gpu, b"allpairs_index", -1)
    E._set(gpu, b"index_join_wgs", 0)


def _grid(gpu, wgs):
    """Sets the grid; -> (waves of the launch, waves the layout is built for)."""
    waves = T._waves(gpu, wgs)
    return waves, (waves if wgs else 8)


def _key(waves, wid, k, j):
    """Key j of the k-th run that wave `wid` of `waves` walks inside a block."""
    return (wid + waves * k) * KRUN + j


def _plant(rng, items, fillers=300):
    """items: (b, u, own, {t: size}): `own` rows in bucket u of block b and size rows in bucket u ^ (1 << t) above it, every
    one a copy of a bucket member with that key bit and (5 m) % 34 bits outside block b flipped: near-duplicates at every
    distance around max_dist inside the bucket and between it and every segment. Fillers stay two bits away."""
    rows, clear = [], {}
    for b, u, own, sizes in items:
        first = T._first(rng, b, u)
        members = [E._flip_outside(rng, first, (3 * m) % 14, {b}) for m in range(own)]
        rows += members
        for t, size in sorted(sizes.items()):
            assert not (u >> t) & 1
            for m in range(size):
                row = E._flip_outside(rng, members[m % own], (5 * m) % 34, {b})
                rows.append(E._flip_bits(row, [E._bit(b, t)]))
        clear.setdefault(b, []).extend([u] + [u ^ (1 << t) for t in range(16)])
    return T._finish(rng, rows, clear, fillers=fillers)


def _ylen(db, b, u):
    return sum(R._ylist(db, b, u))


def _nonempty_items_of_wave(db, waves, wid, world=1, rank=0):
    """The non-empty items of wave `wid`, in the order it walks them."""
    out = []
    for b in range(16):
        counts = np.bincount(E._keys(db, b), minlength=65536)
        for u in np.flatnonzero(counts).tolist():
            it = T._item(b, u)
            if (it // KRUN) % waves == wid and it % world == rank:
                out.append(it)
    return sorted(out)


def _pads(u, need):
    """`need` entries above key u in two segments (key bits 12 and 14: keys of other runs)."""
    assert not (u >> 12) & 1 and not (u >> 14) & 1
    return {12: need // 2, 14: need - need // 2} if need else {}


# ---- 1. neighbours in a wave's sequence

_OTHERS = tuple(x for x in LENGTHS if x != 1)
ORDERS = 15


def _order(k):
    """Eight lengths for the eight keys of two runs, the length 1 on a run's last key. k < 7: the others rotated by k and
    the 1 last; k < 14: the 1 on the first run's last key, so another length is last; 14: as 0, behind a run that holds only
    its last key, with a y list of 1 -- the wave's first non-empty item."""
    r = _OTHERS[k % 7:] + _OTHERS[:k % 7]
    return r + (1,) if k < 7 or k == 14 else r[:3] + (1,) + r[3:]


def _neighbours_db(waves, k, seed):
    """Two consecutive runs of wave 1 in block 2, all eight keys non-empty (one row each), their y lists padded to _order(k)."""
    b, wid = 2, 1
    order = _order(k)
    items = []
    if k == 14:
        items.append((b, _key(waves, wid, 1, KRUN - 1), 1, {}))
    want = {}
    for r, run in enumerate((7, 8)):  # (runs whose numbers, and the lone key's, differ in two bits or more: no neighbours)
        keys = [_key(waves, wid, run, j) for j in range(KRUN)]
        for j in range(KRUN):
            inside = sum(1 for t in range(2) if not (j >> t) & 1)  # one-row buckets above it inside the run
            length = order[4 * r + j]
            assert length >= 1 + inside
            items.append((b, keys[j], 1, _pads(keys[j], length - 1 - inside)))
            want[keys[j]] = length
    for _, u, _, _ in items:
        assert all(v // KRUN == u // KRUN or bin(u ^ v).count("1") >= 2 for _, v, _, _ in items)
    rng = np.random.default_rng(seed)
    return _plant(rng, items), b, wid, want, items


@pytest.mark.parametrize("k", range(ORDERS))
@pytest.mark.parametrize("wgs", GRIDS)
def test_neighbours_in_a_waves_sequence(hvd, gpu, oracle, forced, wgs, k):
    waves, lay = _grid(gpu, wgs)
    db, b, wid, want, items = _neighbours_db(lay, k, seed=10 + k)
    assert KRUN == 4 and sorted(want.values()) == sorted(LENGTHS)
    for u, length in want.items():
        assert _ylen(db, b, u) == length, (hex(u), length)
    planted = sorted(T._item(b, u) for _, u, _, _ in items)
    if k == 14:
        assert _ylen(db, b, items[0][1]) == 1 and T._item(b, items[0][1]) == planted[0]
    if wgs:
        seq = [it for it in _nonempty_items_of_wave(db, waves, wid) if planted[0] <= it <= planted[-1]]
        assert seq == planted  # nothing else of this wave between them: they follow each other
        assert len({T.place(it, waves)[:2] for it in seq}) == 1
    R._check(hvd, gpu, oracle, db)


def test_every_length_is_first_middle_and_last():
    """The orders together: every length of LENGTHS once as the first planted item of the wave, once inside and once as the
    last one; the length 1 always on a key with no non-empty neighbour above it inside its run."""
    firsts, lasts, middles = [], [], set()
    for k in range(ORDERS):
        seq = ((1,) if k == 14 else ()) + _order(k)
        assert sorted(_order(k)) == sorted(LENGTHS) and _order(k).index(1) % KRUN == KRUN - 1
        firsts.append(seq[0]), lasts.append(seq[-1]), middles.update(seq[1:-1])
    assert set(firsts) == set(lasts) == middles == set(LENGTHS)


# ---- 2. gaps: empty items between two non-empty ones

def _gaps_db(waves, kind, seed):
    """Two items of wave 2 with y lists of S + 1 and S + 65 and only empty items of the wave between them: inside a run
    (keys 0 and 3), across the wave's next run (key 2, then key 1 of the next run), across a block boundary (the wave's last
    run of block 5, key 1, then its first run of block 6, key 2)."""
    wid = 2
    if kind == "inside_a_run":
        a, c = (5, _key(waves, wid, 9, 0)), (5, _key(waves, wid, 9, 3))
    elif kind == "next_run":
        a, c = (5, _key(waves, wid, 9, 2)), (5, _key(waves, wid, 10, 1))
    else:
        last = RUNS_PER_BLOCK // waves - 1
        a, c = (5, _key(waves, wid, last, 1)), (6, _key(waves, wid, 0, 2))
    rng = np.random.default_rng(seed)

    def pads(u, need):
        """Up to two segments above u whose keys are not items between the two planted ones: key bit 2 (the next run:
        another wave) or the bits 6 .. 15 (runs far behind)."""
        ts = [t for t in [2] + list(range(6, 16)) if not (u >> t) & 1][:2]
        assert ts
        return {ts[0]: need} if len(ts) == 1 else {ts[0]: need // 2, ts[1]: need - need // 2}
    items = [(a[0], a[1], 3, pads(a[1], S + 1 - 3)), (c[0], c[1], 2, pads(c[1], S + 65 - 2))]
    return _plant(rng, items), wid, a, c


@pytest.mark.parametrize("kind", ["inside_a_run", "next_run", "block_boundary"])
@pytest.mark.parametrize("wgs", GRIDS)
def test_gaps_between_non_empty_items(hvd, gpu, oracle, forced, wgs, kind):
    waves, lay = _grid(gpu, wgs)
    db, wid, a, c = _gaps_db(lay, kind, seed=30 + len(kind))
    assert _ylen(db, *a) == S + 1 and _ylen(db, *c) == S + 65
    if wgs:
        ia, ic = T._item(*a), T._item(*c)
        pa, pc = T.place(ia, waves), T.place(ic, waves)
        assert pa[:2] == pc[:2] == (wid // 4, wid % 4) and pc[2] - pa[2] >= 3  # at least two empty items between them
        seq = _nonempty_items_of_wave(db, waves, wid)
        assert seq.index(ic) == seq.index(ia) + 1  # ... and no non-empty one
        if kind == "inside_a_run":
            assert ia // KRUN == ic // KRUN
        elif kind == "next_run":
            assert ic // KRUN == ia // KRUN + waves
        else:
            assert ia >> 16 == 5 and ic >> 16 == 6 and ic // KRUN == ia // KRUN + waves
    R._check(hvd, gpu, oracle, db)


# ---- 3. bucket sizes of two neighbouring items: whole batches, short last batches, quarters

BUCKETS = (1, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49)


def _buckets_db(waves, own_a, own_c, seed):
    """Keys 2 and 3 of one run of wave 3 in block 9 with buckets of own_a and own_c rows. Every member has, in a bucket
    above its key, one copy at exactly max_dist and one at max_dist + 1 -- so whichever x the counting sort puts first and
    last in the bucket, a pair at 31 and a non-pair at 32 hang on it -- and the y lists are padded to three rounds."""
    b, wid = 9, 3
    rng = np.random.default_rng(seed)
    rows, clear, keys = [], {}, []
    for j, own in ((2, own_a), (3, own_c)):
        u = _key(waves, wid, 6, j)
        first = T._first(rng, b, u)
        members = [E._flip_outside(rng, first, 2 * (m % 6), {b}) for m in range(own)]
        rows += members
        for m, x in enumerate(members):  # key bit 13: one bit of the distance, the others outside the block
            rows.append(E._flip_bits(E._flip_outside(rng, x, 30, {b, b ^ 1}), [E._bit(b, 13)]))
            rows.append(E._flip_bits(E._flip_outside(rng, x, 31, {b, b ^ 1}), [E._bit(b, 13)]))
        pad = max(0, 2 * 64 + 2 - 3 * own - (own_c if j == 2 else 0))
        for m in range(pad):
            rows.append(E._flip_bits(E._flip_outside(rng, members[m % own], (5 * m) % 34, {b}), [E._bit(b, 11)]))
        clear.setdefault(b, []).extend([u] + [u ^ (1 << t) for t in range(16)])
        keys.append(u)
    return T._finish(rng, rows, clear), b, wid, keys


@pytest.mark.parametrize("own_a,own_c", list(zip(BUCKETS, BUCKETS[1:] + BUCKETS[:1])))
@pytest.mark.parametrize("wgs", GRIDS)
def test_bucket_sizes_of_neighbouring_items(hvd, gpu, oracle, forced, wgs, own_a, own_c):
    waves, lay = _grid(gpu, wgs)
    db, b, wid, keys = _buckets_db(lay, own_a, own_c, seed=50 + own_a)
    counts = np.bincount(E._keys(db, b), minlength=65536)
    assert [int(counts[u]) for u in keys] == [own_a, own_c]
    assert all(_ylen(db, b, u) > 2 * 64 for u in keys)  # at least three rounds
    assert keys[1] == keys[0] ^ 1  # neighbouring items, and the second bucket is a segment of the first one's y list
    if wgs:
        pa, pc = T.place(T._item(b, keys[0]), waves), T.place(T._item(b, keys[1]), waves)
        assert pa[:2] == pc[:2] and pc[2] == pa[2] + 1
    want = R._check(hvd, gpu, oracle, db)
    d = want["dist"]
    assert int((d == 31).sum()) >= own_a + own_c  # every member's copy at max_dist came out (the one at 32 is the oracle's to drop)


# ---- 4. ranks

@pytest.mark.parametrize("world", [2, 3, 7])
@pytest.mark.parametrize("wgs", GRIDS)
def test_neighbours_over_the_ranks(hvd, gpu, oracle, forced, wgs, world):
    """The first case's first DB, every rank of the world -- (2, 0), (3, 1) and (7, 6) among them: the union is the oracle's
    list, each pair once."""
    from hvd_amd import multigpu

    _, lay = _grid(gpu, wgs)
    db, _, _, _, _ = _neighbours_db(lay, 0, seed=10)  # (order 0)
    want = oracle.allpairs(db, 31)
    lib = gpu.load()
    d_db = gpu.DeviceBuffer.from_array(db)
    d_img = multigpu.expand_fp4(d_db.ptr, len(db))
    cap = len(want) + 64
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
    assert np.array_equal(np.sort(got, order=["i", "j"]), want), (len(got), len(want))
    assert len(want) >= 8 * S


# ---- 5. drains across items

def _survivor_item(rng, b, u, n, t):
    """Bucket u of block b with n rows whose sibling keys are unrelated, and n rows in bucket u ^ (1 << t), the i-th of
    which shares the word that holds block b with the i-th bucket row up to the key bit -- and nothing else, but for one
    copy at exactly max_dist and one at max_dist + 1: exactly n first-stage survivors, all of item (b, u)."""
    assert not (u >> t) & 1
    sibs = []  # sibling keys pairwise at least four bits apart: no two rows of the bucket survive each other
    while len(sibs) < n:
        c = int(rng.integers(65536))
        if all(bin(c ^ q).count("1") >= 4 for q in sibs):
            sibs.append(c)
    xs = [T._first(rng, b, u) for _ in range(n)]
    for x, q in zip(xs, sibs):
        E._set_key(x[None, :], [0], b ^ 1, q)
    ys = []
    for i, x in enumerate(xs):
        if i == 0:
            y = E._flip_outside(rng, x, 30, {b, b ^ 1})
        elif i == n - 1:
            y = E._flip_outside(rng, x, 31, {b, b ^ 1})
        else:
            y = T._same_word(rng, x, b)
        ys.append(E._flip_bits(y, [E._bit(b, t)]))
    return xs + ys


def _drains_db(waves, n, where, seed):
    """Wave 1: an item of block 4 with n survivors, then in block 8 one with 1 and one with 63 more (`where` "middle"), or
    these two first and the item with n as the wave's last non-empty item, in block 15 (`where` "last")."""
    wid = 1
    rng = np.random.default_rng(seed)
    big = (4, _key(waves, wid, 20, 0)) if where == "middle" else (15, _key(waves, wid, RUNS_PER_BLOCK // waves - 1, 0))
    one, more = (8, _key(waves, wid, 5, 1)), (8, _key(waves, wid, 7, 2))
    rows, clear = [], {}
    for (b, u), cnt in ((big, n), (one, 1), (more, 63)):
        rows += _survivor_item(rng, b, u, cnt, 3)  # (key bit 3: two runs on, another wave's -- nothing of this wave's)
        for key in (u, u ^ (1 << 3)):
            clear.setdefault(b, []).extend([key] + [key ^ (1 << t) for t in range(16)])
    return T._finish(rng, rows, clear, fillers=200), wid, big, one, more


@pytest.mark.parametrize("where", ["middle", "last"])
@pytest.mark.parametrize("n", [64, 65, 127, 128, 129])
@pytest.mark.parametrize("wgs", GRIDS)
def test_drains_across_items(hvd, gpu, oracle, forced, wgs, n, where):
    waves, lay = _grid(gpu, wgs)
    db, wid, big, one, more = _drains_db(lay, n, where, seed=70 + n)
    surv = T._survivors(db)
    assert surv.get(T._item(*big)) == n and surv.get(T._item(*one)) == 1 and surv.get(T._item(*more)) == 63
    if wgs:
        seq = _nonempty_items_of_wave(db, waves, wid)
        # (a pair that shares the word of block b shares the key of its sibling block too: the sibling block's items get a
        # survivor each, one at a time and spread over the waves; the order asserted is that of the three planted items)
        mine = [it for it in seq if it in (T._item(*big), T._item(*one), T._item(*more))]
        want_order = [big, one, more] if where == "middle" else [one, more, big]
        assert mine == [T._item(*x) for x in want_order]
        assert len({it >> 16 for it in mine}) == 2  # the drain that follows the big item mixes two blocks
        if where == "last":
            assert seq[-1] == T._item(*big)
    want = R._check(hvd, gpu, oracle, db)
    assert int((want["dist"] == 31).sum()) >= 2  # (n == 1 plants only the copy at max_dist; the others one at 31 and one at 32)
    if n == 129 and where == "middle":
        # an output buffer shorter than the list: the count is reported, nothing is written past the buffer
        cap, guard = max(1, len(want) // 2), 32
        out = np.zeros(cap + guard, dtype=want.dtype)
        out.view(np.uint8)[:] = 0xA5
        cnt = C.c_int64(0)
        rc = gpu.load().hvd_allpairs_hamming256(db.ctypes.data, len(db), None, 31, out.ctypes.data, cap, C.byref(cnt))
        assert rc == gpu.HVD_ERR_OVERFLOW and cnt.value == len(want) > cap
        assert (out[cap:].view(np.uint8) == 0xA5).all()


# ---- 6. one uniform DB at the default grid

def test_uniform_db_with_planted_near_duplicates(hvd, gpu, oracle, forced):
    rng = np.random.default_rng(90)
    db = rng.integers(0, 256, (30000, 32), dtype=np.uint8)
    src = rng.choice(30000, size=400, replace=False)
    for k in range(200):
        db[src[200 + k]] = E._flip_outside(rng, db[src[k]], (k * 7) % 41, set())
    E._set(gpu, b"index_join_wgs", 0)
    want = R._check(hvd, gpu, oracle, db)
    assert 120 <= len(want) <= 200
