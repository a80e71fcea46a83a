"""The two tile kernels of the pigeonhole index's build: k_index_tile_count (csrc/k_hamming_index.hip), whose workgroups
take their tiles XCD by XCD, and k_index_scatter (csrc/k_index_scatter.hip) on a grid of (tiles, G) block groups per tile,
G = 1, 2 and 4 forced by hvd_debug_set "index_tile_split" -- through hvd_debug_index_tiles (include/hvd_mi355x_bench.h),
which launches the front of the build as a pass does, into buffers of exactly their size with a sentinel tail behind each.
Sizes of 1 .. 17 tiles: fewer tiles than XCDs, a multiple of 8 plus 1, 2 and 4. Every comparison is an equality:
tcnt[part][tile] with a numpy count; ptotal, pbase, pfirst and the chunk list with numpy; rec run by run -- a run is one
(block, partition, tile) -- as multisets with numpy's records AND with what the direct path ("index_stage" 0,
k_index_partition, which the split does not touch) wrote. Sizes 1, 2, one tile less one, one tile, one tile plus one, three
tiles plus 5, 13 tiles plus 1 (14 tiles: six XCDs take two, two take one) and 2^16 + 1 (17 tiles); uniform hashes, all hashes equal (one bin of 4096 staged records per block), and
hashes whose high bytes are all 0xC3, so that one partition of every block takes every tile whole; 300 000 hashes of which
5 000 share a hash, so that partitions are cut into chunks; and one forced search per G against the oracle's brute force."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

TILE, BLOCKS, PARTS = 4096, 16, 4096
MAX_CHUNKS = PARTS + 2048
PART_WORDS = 3 * PARTS + 4 + MAX_CHUNKS  # ptotal, pbase, pfirst (+ 1, padded), chunk_p
GATE_WORD = 12
SPLITS = (1, 2, 4)


def _data(kind, n):
    rng = np.random.default_rng(1000 + n)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if kind == "equal":
        db[:] = db[0]
    elif kind == "one_partition":
        db[:, 1::2] = 0xC3  # little-endian: an odd byte is the high byte of block byte >> 1
    else:
        assert kind == "uniform"
    return db


def _words(db):
    """[n][16] uint32: the word that holds block b with the block's own key in the low half -- a record's second word."""
    w = np.repeat(np.ascontiguousarray(db).view("<u4"), 2, axis=1)
    w[:, 1::2] = w[:, 1::2] >> 16 | w[:, 1::2] << 16
    return w


def _model(db):
    """numpy's tcnt[part][tile] and, per block, the records in run order (partition, then tile, then row)."""
    n = len(db)
    tiles = (n + TILE - 1) // TILE
    w = _words(db)
    high = (w >> 8) & 255
    tile = np.arange(n) // TILE
    tcnt = np.zeros((PARTS, tiles), np.uint32)
    recs = []
    for b in range(BLOCKS):
        np.add.at(tcnt, (b * 256 + high[:, b], tile), 1)
        order = np.argsort(high[:, b], kind="stable")  # (rows ascend inside a partition, so tiles do)
        recs.append(order.astype(np.uint64) | w[order, b].astype(np.uint64) << 32)
    return tcnt, np.stack(recs)


def _parts_model(tcnt, n):
    csz = max(4096, 2 * ((n + 255) // 256))
    ptotal = tcnt.sum(axis=1, dtype=np.uint64).astype(np.uint32)
    per_block = ptotal.reshape(BLOCKS, 256).astype(np.uint64)
    pbase = (np.cumsum(per_block, axis=1) - per_block).reshape(-1).astype(np.uint32)
    nch = (ptotal.astype(np.uint64) + csz - 1) // csz
    pfirst = np.concatenate([[0], np.cumsum(nch)]).astype(np.uint32)
    assert pfirst[-1] <= MAX_CHUNKS
    return ptotal, pbase, pfirst, np.repeat(np.arange(PARTS, dtype=np.uint32), nch.astype(np.int64))


def _run_sorted(rec, run_len):
    """Every run of every block sorted in itself: equal multisets <=> equal arrays."""
    out = np.empty_like(rec)
    for b in range(BLOCKS):
        lens = run_len[b * 256:(b + 1) * 256].reshape(-1)  # (partition-major, then tile: the order of the runs in rec[b])
        out[b] = rec[b][np.lexsort((rec[b], np.repeat(np.arange(lens.size), lens)))]
    return out


def _front(gpu, db, stage, split):
    lib = gpu.ensure()
    fn = lib.hvd_debug_index_tiles  # (bound by hand: include/hvd_mi355x_bench.h)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
    n = len(db)
    tiles = (n + TILE - 1) // TILE
    sel = np.zeros(16, np.uint32)
    sel[GATE_WORD] = 1
    sizes = {"raw": 4 * PARTS * tiles, "tcnt": 4 * PARTS * tiles, "parts": 4 * PART_WORDS, "rec": 8 * BLOCKS * n}
    bufs = {k: _sentinel_buffer(gpu, v) for k, v in sizes.items()}
    d_db, d_sel = gpu.DeviceBuffer.from_array(db), gpu.DeviceBuffer.from_array(sel)
    try:
        gpu.check(lib.hvd_debug_set(b"index_stage", stage))
        gpu.check(lib.hvd_debug_set(b"index_tile_split", split))
        gpu.check(fn(d_db.ptr, n, d_sel.ptr, bufs["raw"].ptr, bufs["tcnt"].ptr, bufs["parts"].ptr, bufs["rec"].ptr))
        gpu.check(lib.hvd_dev_sync())
        out = {k: bufs[k].to_array(np.uint32 if k != "rec" else np.uint64, sizes[k] // (4 if k != "rec" else 8)) for k in sizes}
        for k in sizes:
            assert _tail_intact(gpu, bufs[k], sizes[k]), (k, "overrun", stage, split)
    finally:
        lib.hvd_debug_set(b"index_stage", 1)
        lib.hvd_debug_set(b"index_tile_split", 0)
        for b in list(bufs.values()) + [d_db, d_sel]:
            b.free()
    return out


def _check(gpu, db):
    n = len(db)
    tiles = (n + TILE - 1) // TILE
    tcnt, rec_rows = _model(db)
    ptotal, pbase, pfirst, chunk_p = _parts_model(tcnt, n)
    want = _run_sorted(rec_rows, tcnt)  # (run order: partition-major, as np.repeat over tcnt's rows walks it)
    direct = _run_sorted(_front(gpu, db, 0, 0)["rec"].reshape(BLOCKS, n), tcnt)
    assert np.array_equal(direct, want), "direct path"
    for split in SPLITS:
        got = _front(gpu, db, 1, split)
        bad = np.argwhere(got["raw"].reshape(PARTS, tiles) != tcnt)
        assert bad.size == 0, (split, "tcnt", len(bad), bad[:4].tolist())
        excl = np.cumsum(tcnt, axis=1, dtype=np.uint64).astype(np.uint32) - tcnt
        assert np.array_equal(got["tcnt"].reshape(PARTS, tiles), excl), (split, "tile bases")
        p = got["parts"]
        assert np.array_equal(p[:PARTS], ptotal), (split, "ptotal")
        assert np.array_equal(p[PARTS:2 * PARTS], pbase), (split, "pbase")
        assert np.array_equal(p[2 * PARTS:3 * PARTS + 1], pfirst), (split, "pfirst")
        assert np.array_equal(p[3 * PARTS + 4:3 * PARTS + 4 + len(chunk_p)], chunk_p), (split, "chunk list")
        staged = _run_sorted(got["rec"].reshape(BLOCKS, n), tcnt)
        assert np.array_equal(staged, want), (split, "rec against numpy", int((staged != want).sum()))
        assert np.array_equal(staged, direct), (split, "rec against the direct path")


@pytest.mark.parametrize("kind", ["uniform", "equal", "one_partition"])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 13 * TILE + 1, 65536 + 1])
def test_counts_and_runs_for_every_split(gpu, n, kind):
    _check(gpu, _data(kind, n))


def test_partitions_cut_into_chunks(gpu):
    """300 000 hashes, 5 000 of them one hash: 16 partitions of more than a chunk (4096 entries)."""
    db = _data("uniform", 300_000)
    db[1000:6000] = db[0]
    tcnt, _ = _model(db)
    assert (_parts_model(tcnt, len(db))[0] > 4096).sum() == BLOCKS
    _check(gpu, db)


@pytest.mark.parametrize("split", SPLITS)
def test_forced_search_equals_brute_force(gpu, hvd, oracle, split):
    n = 20_000
    rng = np.random.default_rng(20_000 + split)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for j, k in enumerate(range(0, n - 1, 2)):  # near-duplicates at distances 0 .. 40
        bits = np.unpackbits(db[k])
        bits[rng.choice(256, size=j % 41, replace=False)] ^= 1
        db[k + 1] = np.packbits(bits)
    want = oracle.allpairs(db, 31, num_threads=8)
    assert len(want) > n // 8
    lib = gpu.ensure()
    try:
        gpu.check(lib.hvd_debug_set(b"allpairs_index", 1))
        gpu.check(lib.hvd_debug_set(b"index_tile_split", split))
        got = hvd.allpairs_hamming(db, 31)
        used = C.c_int(0)
        gpu.check(lib.hvd_debug_get(b"allpairs_index_used", C.byref(used)))
    finally:
        lib.hvd_debug_set(b"allpairs_index", -1)
        lib.hvd_debug_set(b"index_tile_split", 0)
    assert used.value == 1
    assert np.array_equal(got, want), (split, len(got), len(want))
