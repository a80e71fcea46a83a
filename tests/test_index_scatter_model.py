"""CPU model of the staged partition pass (csrc/k_index_scatter.hip): per tile and block the records are counted per high
byte, the 256 counts scanned (`lbase`), every record staged at `lbase[h] + rank` -- the ranks inside a bin in any order: on
the device a returning LDS atomic decides -- and staged entry e, whose bin h is read from the record itself, written to
`gbase[h] + (e - lbase[h])` with `gbase[h] = pbase[p] + tcnt[p][tile]`. For every tile and block the written positions must
be a bijection onto the tile's runs as the partition model of tests/test_index_counting_sort_model.py lays them out, and each
run must hold exactly the tile's records of that partition."""
import numpy as np
import pytest

import test_index_counting_sort_model as M

TILE = M.TILE


def run_layout(db, tile=TILE):
    """pbase[part], tbase[part][tile] (the exclusive scan of tcnt over the tiles), tcnt -- the first kernels of M.build_model."""
    n = len(db)
    k = M.keys(db)
    ntiles = (n + tile - 1) // tile
    tcnt = np.zeros((M.N_PARTS, ntiles), dtype=np.int64)
    for t in range(ntiles):
        kt = k[t * tile:(t + 1) * tile]
        for b in range(M.N_BLOCKS):
            tcnt[b * 256:(b + 1) * 256, t] = np.bincount(kt[:, b] >> 8, minlength=256)
    ptotal = tcnt.sum(1)
    tbase = np.cumsum(tcnt, axis=1) - tcnt
    pbase = np.concatenate([np.cumsum(ptotal[b * 256:(b + 1) * 256]) - ptotal[b * 256:(b + 1) * 256] for b in range(M.N_BLOCKS)])
    return pbase, tbase, tcnt


def scatter_model(db, rng, tile=TILE):
    """-> rec_row[16][n], rec_y[16][n] as the staged kernel writes them (-1: never written)."""
    n = len(db)
    k = M.keys(db)
    pbase, tbase, tcnt = run_layout(db, tile)
    ntiles = tcnt.shape[1]
    rec_row = np.full((M.N_BLOCKS, n), -1, dtype=np.int64)
    rec_y = np.zeros((M.N_BLOCKS, n), dtype=np.int64)
    for t in range(ntiles):
        rows = np.arange(t * tile, min(n, (t + 1) * tile))
        held = len(rows)
        for b in range(M.N_BLOCKS):
            key = k[rows, b].astype(np.int64)
            y = key | (k[rows, b ^ 1].astype(np.int64) << 16)  # key of block b | key of its sibling block << 16
            h = key >> 8
            bins = np.bincount(h, minlength=256)
            lbase = np.cumsum(bins) - bins
            # ranks inside a bin: any order
            rank = np.zeros(held, dtype=np.int64)
            cur = np.zeros(256, dtype=np.int64)
            for x in rng.permutation(held):
                rank[x] = cur[h[x]]
                cur[h[x]] += 1
            stage_row = np.full(tile, -1, dtype=np.int64)
            stage_y = np.zeros(tile, dtype=np.int64)
            at = lbase[h] + rank
            assert (at < tile).all() and len(np.unique(at)) == held  # the staged index guard never drops a record
            stage_row[at] = rows
            stage_y[at] = y
            assert (stage_row[:held] >= 0).all()  # the first `held` staged entries are exactly the tile's records
            gbase = pbase[b * 256:(b + 1) * 256] + tbase[b * 256:(b + 1) * 256, t]
            e = np.arange(held)
            he = (stage_y[:held] >> 8) & 255  # from the record itself
            pos = gbase[he] + (e - lbase[he])
            assert (pos >= 0).all() and (pos < n).all()
            assert (rec_row[b, pos] == -1).all() and len(np.unique(pos)) == held  # every slot written once
            rec_row[b, pos] = stage_row[:held]
            rec_y[b, pos] = stage_y[:held]
    return rec_row, rec_y


def check(db, seed=0, tile=TILE):
    rng = np.random.default_rng(seed)
    n = len(db)
    k = M.keys(db)
    rec_row, rec_y = scatter_model(db, rng, tile)
    pbase, tbase, tcnt = run_layout(db, tile)
    assert (rec_row >= 0).all()
    for b in range(M.N_BLOCKS):
        assert np.array_equal(np.sort(rec_row[b]), np.arange(n))  # a bijection onto the block's n positions
        assert np.array_equal(rec_y[b] & 0xFFFF, k[rec_row[b], b])
        assert np.array_equal(rec_y[b] >> 16, k[rec_row[b], b ^ 1])
        for t in range(tcnt.shape[1]):
            lo, hi = t * tile, min(n, (t + 1) * tile)
            for h in np.nonzero(tcnt[b * 256:(b + 1) * 256, t])[0]:
                p = b * 256 + h
                run = rec_row[b, pbase[p] + tbase[p, t]: pbase[p] + tbase[p, t] + tcnt[p, t]]
                want = lo + np.nonzero(k[lo:hi, b] >> 8 == h)[0]
                assert np.array_equal(np.sort(run), want), (b, t, h)  # the run holds exactly the tile's records of the partition
    return rec_row


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


@pytest.mark.parametrize("n", [2, 255, TILE - 1, TILE, 2 * TILE])
def test_uniform_tiles(n):
    check(_uniform(n, n), seed=n)


@pytest.mark.parametrize("last", [1, 17])
def test_short_last_tile(last):
    n = 2 * TILE + last
    check(_uniform(n, last), seed=last)


@pytest.mark.parametrize("block", [0, 15])
def test_one_block_shares_one_high_byte(block):
    # one run of 4096 per whole tile, 255 empty bins
    n = TILE + 600
    db = _uniform(n, 40 + block)
    db[:, 2 * block + 1] = 0xC3
    assert (M.keys(db)[:, block] >> 8 == 0xC3).all()
    check(db, seed=block)


def test_bins_0_and_255_occupied():
    n = TILE + 17
    db = _uniform(n, 7)
    db[::2, 1::2] = 0x00   # every block: half of the rows in bin 0 ...
    db[1::2, 1::2] = 0xFF  # ... and half in bin 255
    hb = M.keys(db) >> 8
    assert set(np.unique(hb)) == {0, 255}
    check(db, seed=7)


def test_the_runs_are_the_partition_models():
    # the partition model (ranks inside a run in any order) and the staged model fill the same runs with the same rows
    n = TILE + 300
    db = _uniform(n, 11)
    rec_row = check(db, seed=11)
    off, rows, kc, cnt, _ = M.build_model(db, np.random.default_rng(11))
    k = M.keys(db)
    for b in range(M.N_BLOCKS):
        # key order of the final index: bucket u = positions off[u] .. off[u + 1]; a partition's region of rec is the union of
        # its buckets' positions, so both hold the same set of rows
        for h in (0, 0xC3, 255):
            lo, hi = off[b, h * 256], off[b, (h + 1) * 256]
            assert np.array_equal(np.sort(rec_row[b, lo:hi]), np.sort(rows[b, lo:hi]))
            assert (k[rec_row[b, lo:hi], b] >> 8 == h).all()
