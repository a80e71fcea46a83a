"""The pigeonhole index path of the auto variant's self all-pairs pass (csrc/k_hamming_index.hip): pair lists equal to the
CPU oracle with the index forced ("allpairs_index" 1) and left to the device's decision (-1), the fallbacks (max_dist 32),
the canonical-block rule (pairs close only in block 15, pairs close in many blocks), skewed and clustered DBs, the group
rule, several contexts on one device (every one of them on the index; a context that cannot get its scratch fails the whole
pass), the overflow contract, and the 1 M headline DB against the matrix-core path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _set(gpu, key, value):
    gpu.check(gpu.load().hvd_debug_set(key, value))


def _get(gpu, key):
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(key, C.byref(v)))
    return v.value


@pytest.fixture
def mode(gpu):
    def set_mode(m):
        _set(gpu, b"allpairs_index", m)

    yield set_mode
    _set(gpu, b"allpairs_index", -1)


def _flip(rng, row, k, bits=None):
    """row with k distinct bits flipped (chosen among `bits` if given)."""
    out = np.unpackbits(row.copy())
    pick = rng.choice(bits if bits is not None else 256, size=k, replace=False)
    out[pick] ^= 1
    return np.packbits(out)


def _planted_db(n, seed, dists=range(0, 41)):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dists = list(dists)
    for k in range(0, n - 1, 2):
        db[k + 1] = _flip(rng, db[k], dists[(k // 2) % len(dists)])
    return db


def _bit(b, t):
    """Packed-hash bit of block b, bit t (block b = bits 16b..16b+15 of the little-endian words; np.unpackbits is MSB first)."""
    byte = 2 * b + t // 8
    return byte * 8 + (7 - t % 8)


def _run(hvd, gpu, db, md, group=None):
    pairs = hvd.allpairs_hamming(db, md, group=group)
    return pairs, _get(gpu, b"allpairs_index_used")


@pytest.mark.parametrize("md", [0, 1, 15, 16, 30, 31])
def test_small_and_odd_sizes_match_the_oracle(hvd, gpu, oracle, mode, md):
    for n in (2, 3, 4, 5, 17, 31, 63, 64, 65, 70, 333, 1001, 4099):
        db = _planted_db(n, seed=n + 100 * md)
        want = oracle.allpairs(db, md)
        for m in (1, -1):
            mode(m)
            got, used = _run(hvd, gpu, db, md)
            assert np.array_equal(got, want), (n, md, m)
            # forced: the index; auto: DBs this small never pay the index's fixed cost
            assert used == (1 if m == 1 else 0), (n, md, m)


def test_tolerance_32_keeps_the_matrix_core_path(hvd, gpu, oracle, mode):
    db = _planted_db(3000, seed=7)
    mode(1)
    got, used = _run(hvd, gpu, db, 32)
    assert used == 0 and np.array_equal(got, oracle.allpairs(db, 32))


def test_pairs_close_only_in_block_15_and_pairs_close_in_many_blocks(hvd, gpu, oracle, mode):
    rng = np.random.default_rng(5)
    n = 4000
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for k in range(0, 1200, 2):
        # blocks 0..14 differ in exactly 2 bits each (30), block 15 in 0 or 1: only block 15 is within r = 1
        row = np.unpackbits(db[k].copy())
        for b in range(15):
            for t in rng.choice(16, size=2, replace=False):
                row[_bit(b, t)] ^= 1
        if k % 4 == 0:
            row[_bit(15, int(rng.integers(16)))] ^= 1
        db[k + 1] = np.packbits(row)
    for k in range(1200, 2400, 2):  # a few flips: close in most blocks at once, must come out once
        db[k + 1] = _flip(rng, db[k], int(rng.integers(0, 9)))
    want = oracle.allpairs(db, 31)
    assert len(want) >= 1200
    mode(1)
    got, used = _run(hvd, gpu, db, 31)
    assert used == 1 and np.array_equal(got, want)
    assert len(np.unique(got[["i", "j"]])) == len(got)


def test_all_identical_db(hvd, gpu, oracle, mode):
    db = np.tile(np.random.default_rng(3).integers(0, 256, (1, 32), dtype=np.uint8), (1500, 1))
    want = oracle.allpairs(db, 31, cap=1500 * 1499 // 2)
    mode(1)
    got, used = _run(hvd, gpu, db, 31)
    assert used == 1 and np.array_equal(got, want)
    mode(-1)
    got, used = _run(hvd, gpu, db, 31)
    assert used == 0 and np.array_equal(got, want)


def test_one_crowded_bucket(hvd, gpu, oracle, mode):
    """5 % of the DB share the key of block 0 (otherwise random): right with the index forced; at 1 M hashes the device keeps
    such a DB on the matrix cores (one wave would walk the crowded bucket alone)."""
    rng = np.random.default_rng(11)
    db = _planted_db(20000, seed=12)
    crowd = rng.choice(20000, size=1000, replace=False)
    db[crowd, 0:2] = 0x5A
    want = oracle.allpairs(db, 31, num_threads=8)
    mode(1)
    got, used = _run(hvd, gpu, db, 31)
    assert used == 1 and np.array_equal(got, want)
    from hvd_amd import synth

    big, _ = synth.hash_db(1_000_000, seed=3)
    big[rng.choice(1_000_000, size=50_000, replace=False), 0:2] = 0x5A
    mode(-1)
    ref = hvd.allpairs_hamming(big, 31)
    assert _get(gpu, b"allpairs_index_used") == 0
    mode(0)
    assert np.array_equal(hvd.allpairs_hamming(big, 31), ref)


@pytest.mark.parametrize("ncl,csz", [(100, 100), (1000, 10)])
def test_clustered_dbs(hvd, gpu, oracle, mode, ncl, csz):
    from hvd_amd import synth

    db, _ = synth.hash_db_clustered(60000, ncl, csz, seed=8)
    want = oracle.allpairs(db, 31, cap=1 << 22, num_threads=8)
    for m in (1, -1):
        mode(m)
        got, _ = _run(hvd, gpu, db, 31)
        assert np.array_equal(got, want), m


def test_group_rule(hvd, gpu, oracle, mode):
    rng = np.random.default_rng(21)
    db = _planted_db(9000, seed=22, dists=range(0, 20))
    group = rng.integers(0, 40, 9000).astype(np.int32)
    group[1::2][: 2000] = group[0::2][: 2000]  # many near pairs inside one group
    for md in (15, 31):
        want = oracle.allpairs(db, md, group=group)
        mode(1)
        got, used = _run(hvd, gpu, db, md, group=group)
        assert used == 1 and np.array_equal(got, want), md


def test_overflow_is_reported_with_the_count(hvd, gpu, oracle, mode):
    db = _planted_db(5000, seed=31, dists=range(0, 10))
    want = oracle.allpairs(db, 31)
    lib = gpu.load()
    mode(1)
    out = np.zeros(10, dtype=gpu.PAIR_DTYPE)
    cnt = C.c_int64(0)
    rc = lib.hvd_allpairs_hamming256(db.ctypes.data, 5000, None, 31, out.ctypes.data, 10, C.byref(cnt))
    assert rc == gpu.HVD_ERR_OVERFLOW and cnt.value == len(want)
    got, used = _run(hvd, gpu, db, 31)
    assert used == 1 and np.array_equal(got, want)


_GROUP_CODE = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np, hvd_amd
from hvd_amd import _lib as L, synth
from oracle import oracle as O
O.build(); lib = L.ensure(); W = L.context_count(); assert W == {w}, W
db, _ = synth.hash_db(30000, seed=9, plant_fraction=0.05)
want = O.allpairs(db, 31, num_threads=8)
def used():
    out = []
    for k in range(W):
        L.set_context(k); v = C.c_int(0); L.check(lib.hvd_debug_get(b"allpairs_index_used", C.byref(v))); out.append(v.value)
    L.set_context(0)
    return out
L.check(lib.hvd_debug_set(b"allpairs_index", 1))
got = hvd_amd.allpairs_hamming(db, 31)
assert np.array_equal(got, want) and len(np.unique(got[["i", "j"]])) == len(got)
assert used() == [1] * W, used()
if {fail_ctx}:
    # one context cannot get its scratch: the pass fails on every rank instead of returning a partial union
    L.check(lib.hvd_debug_set(b"allpairs_index_fail_ctx", {fail_ctx}))
    try:
        hvd_amd.allpairs_hamming(db, 31)
        raise SystemExit("a rank without its index scratch did not fail the pass")
    except L.HvdError:
        pass
    L.check(lib.hvd_debug_set(b"allpairs_index_fail_ctx", 0))
    got = hvd_amd.allpairs_hamming(db, 31)
    assert np.array_equal(got, want) and used() == [1] * W
print("INDEX_GROUP_OK", len(got))
"""


@pytest.mark.parametrize("devs,fail_ctx", [("0,0", 0), ("0,0,0", 2), ("0,0,0,0,0,0,0,0", 7)])
def test_contexts_on_one_device_cover_each_pair_once(devs, fail_ctx):
    code = _GROUP_CODE.format(root=ROOT, w=len(devs.split(",")), fail_ctx=fail_ctx)
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"}
    env["HVD_DEVICES"] = devs
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, text=True)
    assert r.returncode == 0 and "INDEX_GROUP_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_lone_context_without_scratch_falls_back(hvd, gpu, oracle, mode):
    db = _planted_db(5000, seed=41)
    want = oracle.allpairs(db, 31)
    mode(1)
    _set(gpu, b"allpairs_index_fail_ctx", 1)
    try:
        got, used = _run(hvd, gpu, db, 31)
    finally:
        _set(gpu, b"allpairs_index_fail_ctx", 0)
    assert used == 0 and np.array_equal(got, want)
    got, used = _run(hvd, gpu, db, 31)
    assert used == 1 and np.array_equal(got, want)


def test_headline_db_index_equals_matrix_cores(hvd, gpu, mode):
    from hvd_amd import synth

    db, _ = synth.hash_db(1_000_000, seed=3)
    mode(0)
    ref = hvd.allpairs_hamming(db, 31)
    assert _get(gpu, b"allpairs_index_used") == 0
    mode(-1)
    got = hvd.allpairs_hamming(db, 31)
    assert _get(gpu, b"allpairs_index_used") == 1
    assert 2_000_000 < _get(gpu, b"allpairs_index_kcand") < 2_150_000  # exact candidates / 1000 (numpy: 2.075e9)
    assert _get(gpu, b"mfma_auto_form") == 9  # the matrix-core form the probe chose, unchanged
    assert len(got) == 781 and np.array_equal(got, ref)
