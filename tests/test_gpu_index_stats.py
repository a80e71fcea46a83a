"""The statistics kernel of the index build (csrc/k_hamming_index.hip: k_index_stats) against numpy, through the read-outs
"allpairs_index_cand_lo" (the low 31 bits of the exact candidate count) and "allpairs_index_max_walk" (the longest work item,
saturated at 2^32 - 1 on the device and reported as at most 2^31 - 1), after one auto-variant `allpairs_hamming` call. The
numpy side: `candidate_count` of tests/test_allpairs_index_model.py and, on its own, the maximum over (block, key u) of
c_u (c_u + r x the counts of the one-bit neighbours above u).

The statistics run only in a pass that is eligible for the index and whose probe lets the histograms be built; a pass over a
DB as small as these is not eligible on its own (csrc/k_hamming_index.hip: index_eligible), so the read-outs are taken from a
pass with the index forced ("allpairs_index" 1) and the device's own decision from a second pass with "allpairs_index" -1.
Cases: 3001 uniform hashes at tolerances 31 (r = 1) and 15 (r = 0); a DB in which the keys 0x0000 (16 neighbours above it)
and 0xFFFF (none) of one block are occupied, with occupied neighbours on both sides; 20 000 hashes of which 1000 share block
0's key, where the longest walk is that bucket's and the device's own pass does not use the index; 70 000 hashes that share
block 3's key and nothing else, where c^2 > 2^32 saturates the walk, the read-out is 2^31 - 1, the device's own pass falls
back and its pair list equals the one with the index switched off. Every GPU step is a child process of its own under a time
limit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_HEAD = """
import ctypes as C, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, hvd_amd
from hvd_amd import _lib as L
from test_allpairs_index_model import candidate_count, keys, radius
lib = L.ensure()
def mode(m): L.check(lib.hvd_debug_set(b"allpairs_index", m))
def get(key):
    v = C.c_int(0); L.check(lib.hvd_debug_get(key, C.byref(v))); return v.value
def numpy_walk(db, r):
    k, best = keys(db), 0
    u = np.arange(1 << 16)
    for b in range(16):
        c = np.bincount(k[:, b], minlength=1 << 16).astype(np.int64)
        above = np.zeros_like(c)
        for t in range(16):
            above += np.where((u >> t) & 1 == 0, c[u ^ (1 << t)], 0)
        best = max(best, int((c * (c + r * above)).max()))
    return best
def stats(db, md, want_used=1):
    # -> the forced pass's pair list; the read-outs checked against numpy
    r = radius(md)
    total, walk = candidate_count(db, r)
    assert walk == numpy_walk(db, r)
    mode(1)
    got = hvd_amd.allpairs_hamming(db, md)
    assert get(b"allpairs_index_used") == want_used
    lo, mw = get(b"allpairs_index_cand_lo"), get(b"allpairs_index_max_walk")
    print("cand", total, "cand_lo", lo, "walk", walk, "max_walk", mw, flush=True)
    if total < 2 ** 31:
        assert lo == total, (lo, total)
        assert get(b"allpairs_index_kcand") == total // 1000
    else:
        assert lo == total & 0x7FFFFFFF, (lo, total)  # (the count itself does not fit the read-out: its low 31 bits do)
    assert mw == min(walk, 2 ** 31 - 1), (mw, walk)
    mode(-1)
    return got, total, walk
"""

_UNIFORM = _HEAD + """
db = np.random.default_rng(3001).integers(0, 256, (3001, 32), dtype=np.uint8)
for md in (31, 15):
    _, total, walk = stats(db, md)
    assert 0 < total < 2 ** 31 and walk > 0
print("STATS_OK")
"""

_CORNER_KEYS = _HEAD + """
rng = np.random.default_rng(77)
db = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
B = 5
def put(rows, key): db[rows, 2 * B] = key & 255; db[rows, 2 * B + 1] = key >> 8
at = 0
def take(k):
    global at
    at += k
    return slice(at - k, at)
put(take(40), 0x0000)
put(take(50), 0xFFFF)
for t in range(16):
    put(take(3 + t % 2), 1 << t)           # the 16 neighbours above key 0
    put(take(5), 0xFFFF ^ (1 << t))        # the 16 keys below 0xFFFF: it is THEIR neighbour above, and has none itself
c = np.bincount(keys(db)[:, B], minlength=1 << 16)
assert c[0] >= 40 and c[0xFFFF] >= 50
for md in (31, 15):
    _, total, walk = stats(db, md)
    assert total < 2 ** 31
    # key 0: 16 neighbours above it; key 0xFFFF: none -- the longest walk of the DB is one of the two, by construction
    w0 = int(c[0]) * (int(c[0]) + radius(md) * int(sum(c[1 << t] for t in range(16))))
    w1 = int(c[0xFFFF]) ** 2
    assert walk == max(w0, w1), (walk, w0, w1)
print("STATS_OK")
"""

_CROWDED = _HEAD + """
rng = np.random.default_rng(20)
db = rng.integers(0, 256, (20000, 32), dtype=np.uint8)
crowd = rng.choice(20000, size=1000, replace=False)
db[crowd, 0:2] = 0x5A
got, total, walk = stats(db, 31)
assert total < 2 ** 31
assert 1000 * 1000 <= walk < 1000 * 1100  # the crowded bucket's walk is the longest by far (a uniform bucket holds ~0.3 rows)
ref = hvd_amd.allpairs_hamming(db, 31)  # the device's own decision
assert get(b"allpairs_index_used") == 0
assert np.array_equal(got, ref)
print("STATS_OK")
"""

_SATURATED = _HEAD + """
rng = np.random.default_rng(70)
n = 70000
db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
db[:, 6:8] = (0x3C, 0xA5)  # block 3's key, shared by every row; every other block is uniform
got, total, walk = stats(db, 31)
assert walk >= n * n > 2 ** 32 and total >= n * (n - 1) // 2 > 2 ** 31  # the walk saturates; only the low bits of the count are read
ref = hvd_amd.allpairs_hamming(db, 31)  # the device's own decision: the pass falls back
assert get(b"allpairs_index_used") == 0
mode(0)
off = hvd_amd.allpairs_hamming(db, 31)
mode(-1)
assert np.array_equal(ref, off) and np.array_equal(got, off), (len(got), len(ref), len(off))
print("STATS_OK")
"""


def _child(code, seconds):
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=seconds, text=True)
    assert r.returncode == 0 and "STATS_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


def test_uniform_hashes_at_both_radii():
    _child(_UNIFORM.format(root=ROOT), 240)


def test_keys_0x0000_and_0xffff_of_one_block():
    _child(_CORNER_KEYS.format(root=ROOT), 240)


def test_crowded_bucket_sets_the_longest_walk_and_the_pass_stays_off_the_index():
    _child(_CROWDED.format(root=ROOT), 240)


def test_walk_saturates_and_the_pass_falls_back():
    _child(_SATURATED.format(root=ROOT), 240)
