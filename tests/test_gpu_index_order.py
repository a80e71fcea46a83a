"""Partitions ordered whole in LDS (csrc/k_index_order.hip) next to partitions ordered by chunks (csrc/k_hamming_index.hip), with
the index forced: pair lists equal to the CPU oracle, every (i, j) at most once, at tolerances 31 and 15. DBs of kOrderMax + 600
rows in which exactly k rows share the high byte 0xC3 of one block's key and no other row has it, for k = kOrderMax - 1,
kOrderMax (the workgroup's LDS arrays exactly full) and kOrderMax + 1 (that partition takes the chunk path while every other
partition of the same pass is ordered whole): block 0 (byte 1) and block 15 (byte 31); the same with the low byte shared too,
so that one bin holds the whole partition; and n = 255, where nearly every partition is empty. Every GPU step is a child
process of its own under a time limit."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_HDR = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "hvd_index_dev.h")
ORDER_MAX = int(re.search(r"constexpr uint32_t kOrderMax = (\d+);", open(_HDR).read()).group(1))

_HEAD = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np, hvd_amd
from hvd_amd import _lib as L
from oracle import oracle as O
O.build(); lib = L.ensure()
def used():
    v = C.c_int(0); L.check(lib.hvd_debug_get(b"allpairs_index_used", C.byref(v))); return v.value
def flip(rng, row, k):
    out = np.unpackbits(row.copy()); out[rng.choice(256, size=k, replace=False)] ^= 1
    return np.packbits(out)
def planted(n, seed, step=2):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for j, k in enumerate(range(0, n - 1, step)):
        db[k + 1] = flip(rng, db[k], j % 41)  # near-duplicates at distances 0 .. 40
    return db
def check(db, what):
    for md in (31, 15):
        want = O.allpairs(db, md, num_threads=8)
        got = hvd_amd.allpairs_hamming(db, md)
        assert used() == 1, (what, md)
        assert len(np.unique(got[["i", "j"]])) == len(got), (what, md)
        assert len(want) > len(db) // 8 and np.array_equal(got, want), (what, md, len(got), len(want))
L.check(lib.hvd_debug_set(b"allpairs_index", 1))
"""

_AT_THE_CAP = _HEAD + """
cap, byte, low = {cap}, {byte}, {low}
n = cap + 600
for k in {ks}:
    db = planted(n, seed=1000 * byte + k)
    hi = db[:, byte]
    hi[hi == 0xC3] = 0x3C
    hi[:k] = 0xC3  # exactly k rows in partition (byte >> 1, 0xC3), most of them planted pairs of each other
    if low:
        db[:k, byte - 1] = 0x5A  # ... and all of them in one bucket
    assert int((db[:, byte] == 0xC3).sum()) == k
    check(db, k)
print("ORDER_OK", n)
"""

_TINY = _HEAD + """
check(planted(255, seed=255), 255)
print("ORDER_OK", 255)
"""


def _child(code, seconds):
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=seconds, text=True)
    assert r.returncode == 0 and "ORDER_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("byte", [1, 31])
def test_one_partition_below_at_and_above_the_cap(byte):
    ks = (ORDER_MAX - 1, ORDER_MAX, ORDER_MAX + 1)
    _child(_AT_THE_CAP.format(root=ROOT, cap=ORDER_MAX, byte=byte, low=0, ks=ks), 240)


def test_one_bin_holds_the_whole_partition():
    _child(_AT_THE_CAP.format(root=ROOT, cap=ORDER_MAX, byte=1, low=1, ks=(ORDER_MAX, ORDER_MAX + 1)), 240)


def test_nearly_every_partition_is_empty():
    _child(_TINY.format(root=ROOT), 240)
