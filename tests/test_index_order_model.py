"""CPU model of the index build with its two low-byte paths (csrc/k_index_order.hip next to csrc/k_hamming_index.hip): the
high-byte partition pass as test_index_counting_sort_model states it, then every partition of 1 .. cap records ordered WHOLE
(count, scan, rank, laid out in final order, copied out: k_index_order) and every larger one by CHUNKS (k_index_count,
k_index_offsets, k_index_place, which skip what the other path took; an empty partition gets its zero counts from
k_index_offsets). One size test decides, as on the device (hvd_index_dev.h: orders_whole). `off` must be the cumulative
bincount of each block's keys and every bucket must hold exactly its rows, at caps that put the split inside the DBs; the
ranks inside a run come in random order (on the device the LDS atomics decide)."""
import os
import re

import numpy as np
import pytest

import test_index_counting_sort_model as M

N_BLOCKS, N_KEYS, N_PARTS, TILE = M.N_BLOCKS, M.N_KEYS, M.N_PARTS, M.TILE
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc",
                    "hvd_index_dev.h")
ORDER_MAX = int(re.search(r"constexpr uint32_t kOrderMax = (\d+);", open(_HDR).read()).group(1))


def orders_whole(records, cap):
    return 1 <= records <= cap


def build_model(db, rng, cap, tile=TILE, csz=None):
    """-> off[16][65537], rows[16][n], key copies[16][n], cnt[16][65536], partitions ordered whole, chunks that did work"""
    n = len(db)
    k = M.keys(db)
    csz = csz or M.chunk_size(n)
    ntiles = (n + tile - 1) // tile
    # k_index_tile_count, k_index_scan_rows, k_index_scan_parts
    tcnt = np.zeros((N_PARTS, ntiles), dtype=np.int64)
    for t in range(ntiles):
        kt = k[t * tile:(t + 1) * tile]
        for b in range(N_BLOCKS):
            tcnt[b * 256:(b + 1) * 256, t] = np.bincount(kt[:, b] >> 8, minlength=256)
    ptotal = tcnt.sum(1)
    tbase = np.cumsum(tcnt, axis=1) - tcnt
    pbase = np.concatenate([np.cumsum(ptotal[b * 256:(b + 1) * 256]) - ptotal[b * 256:(b + 1) * 256] for b in range(N_BLOCKS)])
    nch = (ptotal + csz - 1) // csz
    pfirst = np.concatenate([[0], np.cumsum(nch)])
    chunk_p = np.repeat(np.arange(N_PARTS), nch)
    # k_index_partition
    rec_row = np.full((N_BLOCKS, n), -1, dtype=np.int64)
    rec_key = np.zeros((N_BLOCKS, n), dtype=np.int64)
    for t in range(ntiles):
        cur = pbase + tbase[:, t]
        for i in rng.permutation(np.arange(t * tile, min(n, (t + 1) * tile))):
            for b in range(N_BLOCKS):
                p = b * 256 + (k[i, b] >> 8)
                rec_row[b, cur[p]] = i
                rec_key[b, cur[p]] = k[i, b]
                cur[p] += 1
    assert (rec_row >= 0).all()

    NONE = -1
    off = np.full((N_BLOCKS, N_KEYS + 1), NONE, dtype=np.int64)
    cnt = np.full((N_BLOCKS, N_KEYS), NONE, dtype=np.int64)
    rows = np.full((N_BLOCKS, n), NONE, dtype=np.int64)
    kc = np.full((N_BLOCKS, n), NONE, dtype=np.int64)

    def write_keys(p, total, pos):  # what thread t = key h * 256 + t writes, in either kernel: once per key
        b, h = p >> 8, p & 255
        assert (cnt[b, h * 256:(h + 1) * 256] == NONE).all() and (off[b, h * 256:(h + 1) * 256] == NONE).all()
        cnt[b, h * 256:(h + 1) * 256] = total
        off[b, h * 256:(h + 1) * 256] = pos
        if h == 255:
            off[b, N_KEYS] = n

    # k_index_order: one workgroup per partition
    whole = 0
    for p in range(N_PARTS):
        if not orders_whole(ptotal[p], cap):
            continue
        whole += 1
        b = p >> 8
        lo, hi = pbase[p], pbase[p] + ptotal[p]
        count = np.bincount(rec_key[b, lo:hi] & 255, minlength=256)
        cur = np.cumsum(count) - count  # inside the partition
        write_keys(p, count, pbase[p] + cur)
        lds_key = np.full(ptotal[p], NONE, dtype=np.int64)
        lds_row = np.full(ptotal[p], NONE, dtype=np.int64)
        cur = cur.copy()
        for e in rng.permutation(np.arange(lo, hi)):
            low = rec_key[b, e] & 255
            assert lds_row[cur[low]] == NONE
            lds_key[cur[low]], lds_row[cur[low]] = rec_key[b, e], rec_row[b, e]
            cur[low] += 1
        assert (rows[b, lo:hi] == NONE).all()
        rows[b, lo:hi], kc[b, lo:hi] = lds_row, lds_key  # the two contiguous streams

    def chunk(c):  # chunk_of: None for a chunk of a partition that was ordered whole
        p = chunk_p[c]
        if orders_whole(ptotal[p], cap):
            return None
        lo = (c - pfirst[p]) * csz
        return p, p >> 8, pbase[p] + lo, pbase[p] + min(ptotal[p], lo + csz)

    # k_index_count
    ccount = np.full((len(chunk_p), 256), NONE, dtype=np.int64)  # (a skipped chunk's counters stay unwritten and unread)
    worked = 0
    for c in range(len(chunk_p)):
        q = chunk(c)
        if q is None:
            continue
        worked += 1
        p, b, lo, hi = q
        ccount[c] = np.bincount(rec_key[b, lo:hi] & 255, minlength=256)
    # k_index_offsets
    for p in range(N_PARTS):
        if orders_whole(ptotal[p], cap):
            continue
        mine = ccount[pfirst[p]:pfirst[p + 1]]
        assert (mine != NONE).all()
        total = mine.sum(0) if nch[p] else np.zeros(256, dtype=np.int64)
        pos = pbase[p] + np.cumsum(total) - total
        write_keys(p, total, pos)
        for c in range(pfirst[p], pfirst[p + 1]):
            v = ccount[c].copy()
            ccount[c] = pos
            pos = pos + v
    # k_index_place
    for c in range(len(chunk_p)):
        q = chunk(c)
        if q is None:
            continue
        p, b, lo, hi = q
        cur = ccount[c].copy()
        for e in rng.permutation(np.arange(lo, hi)):
            low = rec_key[b, e] & 255
            assert rows[b, cur[low]] == NONE
            rows[b, cur[low]] = rec_row[b, e]
            kc[b, cur[low]] = rec_key[b, e]
            cur[low] += 1
    return off, rows, kc, cnt, whole, worked


def check(db, cap, seed=0, **kw):
    rng = np.random.default_rng(seed)
    off, rows, kc, cnt, whole, worked = build_model(db, rng, cap, **kw)
    k = M.keys(db)
    n = len(db)
    for b in range(N_BLOCKS):
        c = np.bincount(k[:, b], minlength=N_KEYS)
        assert np.array_equal(cnt[b], c)
        assert np.array_equal(off[b], np.concatenate([[0], np.cumsum(c)]))
        assert np.array_equal(np.sort(rows[b]), np.arange(n))  # every row once
        assert np.array_equal(k[rows[b], b], kc[b])            # the copy next to a row is that row's
        assert (np.diff(kc[b]) >= 0).all()                     # key order: bucket u = positions off[u] .. off[u + 1]
    return whole, worked


def test_the_device_cap_fits_lds_and_covers_a_uniform_db():
    assert 8 * ORDER_MAX + 4 * 256 + 16 <= 64 * 1024
    assert ORDER_MAX >= 4096 + 10 * 64  # 2^20 uniform hashes: partitions of 4096 +- 64 records


# random DBs of n hashes: partitions of about n / 256 records, sd sqrt(n / 256) -- caps below, inside and above that spread
@pytest.mark.parametrize("n,cap", [(255, 4), (1000, 3), (1000, 4), (1000, 10**6), (TILE + 1, 12), (TILE + 1, 16), (TILE + 1, 20),
                                   (3 * TILE + 17, 48)])
def test_random_dbs_split_between_the_two_paths(n, cap):
    db = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
    sizes = np.concatenate([np.bincount(M.keys(db)[:, b] >> 8, minlength=256) for b in range(N_BLOCKS)])
    whole, worked = check(db, cap, seed=n + cap)
    assert whole == ((sizes >= 1) & (sizes <= cap)).sum()
    if cap < 10**6:
        assert 0 < whole < (sizes >= 1).sum() and worked > 0  # the split is inside the DB
    else:
        assert worked == 0


@pytest.mark.parametrize("k", [299, 300, 301])
@pytest.mark.parametrize("block", [0, 15])
def test_one_partition_at_the_cap(block, k):
    """exactly k rows share the high byte 0xC3 of the block's key: whole at k <= cap = 300, by chunks at 301 -- while every
    other partition of the pass (a few records each) is ordered whole"""
    n, cap = 900, 300
    rng = np.random.default_rng(k + block)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    hi = db[:, 2 * block + 1]
    hi[hi == 0xC3] = 0x3C
    hi[rng.choice(n, size=k, replace=False)] = 0xC3
    assert (M.keys(db)[:, block] >> 8 == 0xC3).sum() == k
    whole, worked = check(db, cap, seed=k, csz=128)
    assert worked == (0 if k <= cap else -(-k // 128))


def test_one_bin_holds_the_whole_partition():
    n, cap, k = 900, 300, 300
    rng = np.random.default_rng(9)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    db[db[:, 1] == 0xC3, 1] = 0x3C
    sel = rng.choice(n, size=k, replace=False)
    db[sel, 1], db[sel, 0] = 0xC3, 0x5A  # one key: high and low byte
    whole, worked = check(db, cap, seed=2)
    assert worked == 0


def test_all_identical_db_takes_the_chunks():
    n = 1500
    db = np.tile(np.random.default_rng(3).integers(0, 256, (1, 32), dtype=np.uint8), (n, 1))
    whole, worked = check(db, cap=1499, seed=4)
    assert whole == 0 and worked == 16 * -(-n // M.chunk_size(n))
    whole, worked = check(db, cap=1500, seed=4)
    assert whole == 16 and worked == 0
