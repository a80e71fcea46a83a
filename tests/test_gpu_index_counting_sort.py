"""The index build as a two-level counting sort (csrc/k_hamming_index.hip), with the index forced: pair lists equal to the
CPU oracle at sizes around 256 and around the tile, a DB whose block-0 keys share one high byte (one partition holds every
hash: far larger than LDS, cut into chunks), and the same pass from two contexts on one device. Every GPU step is a child
process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE = 4096  # kTile

_HEAD = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np, hvd_amd
from hvd_amd import _lib as L
from oracle import oracle as O
O.build(); lib = L.ensure()
def mode(m): L.check(lib.hvd_debug_set(b"allpairs_index", m))
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
"""

_SIZES = _HEAD + """
n = {n}
db = planted(n, seed=n, step=2 if n < 50000 else 40)
for md in (31, 15):
    want = O.allpairs(db, md, num_threads=8)
    mode(1)
    got = hvd_amd.allpairs_hamming(db, md)
    assert used() == 1, md
    assert np.array_equal(got, want), (n, md, len(got), len(want))
print("SORT_OK", n, len(got))
"""

_ONE_PARTITION = _HEAD + """
n = 300000
db = planted(n, seed=77, step=40)
db[:, 1] = 0xC3  # the high byte of every key of block 0: one partition of n entries
db[: n // 100, 0] = 0x11  # and 1 % of them in one bucket
mode(0)
ref = hvd_amd.allpairs_hamming(db, 31)
assert used() == 0
mode(1)
got = hvd_amd.allpairs_hamming(db, 31)
assert used() == 1
assert len(ref) > 3000 and np.array_equal(got, ref), (len(got), len(ref))
print("SORT_OK", n, len(got))
"""

_TWO_CONTEXTS = _HEAD + """
W = L.context_count(); assert W == 2, W
db = planted(3 * {tile} + 17, seed=5)
want = O.allpairs(db, 31, num_threads=8)
mode(1)
for _ in range(2):
    got = hvd_amd.allpairs_hamming(db, 31)
    assert np.array_equal(got, want) and len(np.unique(got[["i", "j"]])) == len(got)
    for k in range(W):
        L.set_context(k); assert used() == 1, k
    L.set_context(0)
print("SORT_OK", len(db), len(got))
"""


def _child(code, seconds, devices=None):
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"} if devices else dict(os.environ)
    if devices:
        env["HVD_DEVICES"] = devices
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=seconds, text=True)
    assert r.returncode == 0 and "SORT_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("n", [2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 200_001])
def test_forced_index_matches_the_oracle(n):
    _child(_SIZES.format(root=ROOT, n=n), 600 if n > 100_000 else 240)


def test_one_partition_holds_every_hash():
    _child(_ONE_PARTITION.format(root=ROOT), 600)


def test_two_contexts_on_one_device():
    _child(_TWO_CONTEXTS.format(root=ROOT, tile=TILE), 300, devices="0,0")
