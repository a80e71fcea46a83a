"""CPU model of the index build (csrc/k_hamming_index.hip): a two-level counting sort of every block's 16-bit keys --
tile counts of the high byte, scan over the tiles and over the partitions, partition records, chunked low-byte counts,
offsets and cursors, place. Its `off` must be the cumulative bincount of each block's keys and every bucket must hold exactly
the rows with that key, whatever order the ranks inside a run come in (the model draws them at random: on the device the
LDS atomics decide)."""
import numpy as np
import pytest

N_BLOCKS, N_KEYS, N_PARTS = 16, 1 << 16, 16 * 256
TILE = 4096          # kTile
MIN_CHUNK = 4096     # kMinChunk
MAX_CHUNKS = N_PARTS + 2048  # kMaxChunks


def keys(db):
    return np.ascontiguousarray(db).view("<u2").astype(np.uint32)


def chunk_size(n):
    return max(MIN_CHUNK, 2 * ((n + 255) // 256))


def build_model(db, rng, tile=TILE, csz=None):
    """-> off[16][65537], rows[16][n], key copies[16][n] (the device keeps the 32-byte hash there), chunks used."""
    n = len(db)
    k = keys(db)
    csz = csz or chunk_size(n)
    ntiles = (n + tile - 1) // tile
    # k_index_tile_count: tcnt[part][tile]
    tcnt = np.zeros((N_PARTS, ntiles), dtype=np.int64)
    for t in range(ntiles):
        kt = k[t * tile:(t + 1) * tile]
        for b in range(N_BLOCKS):
            tcnt[b * 256:(b + 1) * 256, t] = np.bincount(kt[:, b] >> 8, minlength=256)
    # k_index_scan_rows
    ptotal = tcnt.sum(1)
    tbase = np.cumsum(tcnt, axis=1) - tcnt
    # k_index_scan_parts
    pbase = np.concatenate([np.cumsum(ptotal[b * 256:(b + 1) * 256]) - ptotal[b * 256:(b + 1) * 256] for b in range(N_BLOCKS)])
    nch = (ptotal + csz - 1) // csz
    pfirst = np.concatenate([[0], np.cumsum(nch)])
    assert pfirst[-1] <= MAX_CHUNKS
    chunk_p = np.repeat(np.arange(N_PARTS), nch)
    # k_index_partition: rank inside the tile's run in any order
    rec_row = np.full((N_BLOCKS, n), -1, dtype=np.int64)
    rec_key = np.zeros((N_BLOCKS, n), dtype=np.int64)
    for t in range(ntiles):
        cur = pbase + tbase[:, t]
        for i in rng.permutation(np.arange(t * tile, min(n, (t + 1) * tile))):
            for b in range(N_BLOCKS):
                p = b * 256 + (k[i, b] >> 8)
                assert rec_row[b, cur[p]] == -1  # every record slot is written once
                rec_row[b, cur[p]] = i
                rec_key[b, cur[p]] = k[i, b]
                cur[p] += 1
    assert (rec_row >= 0).all()

    def chunk(c):
        p = chunk_p[c]
        lo = (c - pfirst[p]) * csz
        return p, p >> 8, pbase[p] + lo, pbase[p] + min(ptotal[p], lo + csz)

    # k_index_count
    ccount = np.zeros((len(chunk_p), 256), dtype=np.int64)
    for c in range(len(chunk_p)):
        p, b, lo, hi = chunk(c)
        assert ((rec_key[b, lo:hi] >> 8) == (p & 255)).all()
        ccount[c] = np.bincount(rec_key[b, lo:hi] & 255, minlength=256)
    # k_index_offsets
    off = np.zeros((N_BLOCKS, N_KEYS + 1), dtype=np.int64)
    cnt = np.zeros((N_BLOCKS, N_KEYS), dtype=np.int64)
    for p in range(N_PARTS):
        b, h = p >> 8, p & 255
        total = ccount[pfirst[p]:pfirst[p + 1]].sum(0) if nch[p] else np.zeros(256, dtype=np.int64)
        pos = pbase[p] + np.cumsum(total) - total
        cnt[b, h * 256:(h + 1) * 256] = total
        off[b, h * 256:(h + 1) * 256] = pos
        for c in range(pfirst[p], pfirst[p + 1]):
            v = ccount[c].copy()
            ccount[c] = pos
            pos = pos + v
    off[:, N_KEYS] = n
    # k_index_place
    rows = np.full((N_BLOCKS, n), -1, dtype=np.int64)
    kc = np.zeros((N_BLOCKS, n), dtype=np.int64)
    for c in range(len(chunk_p)):
        p, b, lo, hi = chunk(c)
        cur = ccount[c].copy()
        for e in rng.permutation(np.arange(lo, hi)):
            low = rec_key[b, e] & 255
            assert rows[b, cur[low]] == -1
            rows[b, cur[low]] = rec_row[b, e]
            kc[b, cur[low]] = rec_key[b, e]
            cur[low] += 1
    return off, rows, kc, cnt, len(chunk_p)


def check(db, seed=0, **kw):
    rng = np.random.default_rng(seed)
    off, rows, kc, cnt, nchunks = build_model(db, rng, **kw)
    k = keys(db)
    n = len(db)
    for b in range(N_BLOCKS):
        c = np.bincount(k[:, b], minlength=N_KEYS)
        assert np.array_equal(cnt[b], c)
        assert np.array_equal(off[b], np.concatenate([[0], np.cumsum(c)]))
        assert np.array_equal(np.sort(rows[b]), np.arange(n))  # every row once
        assert np.array_equal(k[rows[b], b], kc[b])            # the copy next to a row is that row's
        assert (np.diff(kc[b]) >= 0).all()                     # key order: bucket u = positions off[u] .. off[u + 1]
    return nchunks


@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 1000, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_random_dbs(n):
    db = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
    check(db, seed=n)


@pytest.mark.parametrize("n", [2, 256, 1500, TILE + 1])
def test_all_identical_db(n):
    db = np.tile(np.random.default_rng(3).integers(0, 256, (1, 32), dtype=np.uint8), (n, 1))
    assert check(db) == 16 * -(-n // chunk_size(n))  # one partition per block, cut into chunks


@pytest.mark.parametrize("block", [0, 7, 15])
def test_every_key_of_a_block_shares_its_high_byte(block):
    n = 2 * TILE + 300
    db = np.random.default_rng(block).integers(0, 256, (n, 32), dtype=np.uint8)
    db[:, 2 * block + 1] = 0xC3  # little-endian: the second byte of the block is the key's high byte
    assert (keys(db)[:, block] >> 8 == 0xC3).all()
    # the partition holds all n entries: 3 chunks of 4096 here
    check(db, seed=block)


def test_one_partition_split_over_many_chunks():
    n = 5000
    db = np.random.default_rng(8).integers(0, 256, (n, 32), dtype=np.uint8)
    db[:, 1] = 0x11
    db[: n // 2, 0] = 0x22  # and half of them in one bucket
    nchunks = check(db, seed=1, tile=512, csz=300)
    assert nchunks > 16 * 17  # block 0: ceil(5000 / 300) = 17 chunks of one partition


def test_chunk_bound():
    # sum over partitions of ceil(size / csz) <= 4096 + 16 n / csz <= 4096 + 2048 for every n
    for n in (2, 4095, 4096, 100_000, 524_288, 524_289, 1_000_000, 10_000_000, 2 ** 32 - 1):
        assert N_PARTS + (16 * n) // chunk_size(n) <= MAX_CHUNKS, n
