"""The staged partition pass (csrc/k_index_scatter.hip, "index_stage" 1: a tile's runs laid out in LDS and copied out in
order) next to the direct one (k_index_partition, "index_stage" 0), with the index forced, at tolerances 31 and 15: for each
DB the two pair lists and the CPU oracle's brute force are equal, every (i, j) appears at most once and the pass ran on the
index. DBs with planted near-duplicates at distances 0 .. 40 (as tests/test_gpu_index_order.py), of 2, 255, 4095, 4096, 4097
and 2 x 4096 + 17 rows (three tiles, the last of 17); 4097 + 600 rows that all share the high byte 0xC3 of block 0's key, so
that one partition takes whole tiles (one bin of 4096 staged records, 255 empty ones), the same for block 15, and with every
odd byte constant, so that every block has one occupied bin; and the three-tile DB from two contexts on one device. Every GPU
step is a child process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE = 4096

_HEAD = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np, hvd_amd
from hvd_amd import _lib as L
from oracle import oracle as O
O.build(); lib = L.ensure(); W = L.context_count()
def used():
    out = []
    for k in range(W):
        if W > 1: L.set_context(k)
        v = C.c_int(0); L.check(lib.hvd_debug_get(b"allpairs_index_used", C.byref(v))); out.append(v.value)
    if W > 1: L.set_context(0)
    return out
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
    n = len(db)
    for md in (31, 15):
        want = O.allpairs(db, md, num_threads=8)
        assert len(want) > 0 and (n < 255 or len(want) > n // 8), (what, md, len(want))
        got = {{}}
        for stage in (1, 0):
            L.check(lib.hvd_debug_set(b"index_stage", stage))
            got[stage] = hvd_amd.allpairs_hamming(db, md)
            assert used() == [1] * W, (what, md, stage, used())
            assert len(np.unique(got[stage][["i", "j"]])) == len(got[stage]), (what, md, stage)
        L.check(lib.hvd_debug_set(b"index_stage", 1))
        assert np.array_equal(got[1], want), (what, md, "staged", len(got[1]), len(want))
        assert np.array_equal(got[0], want), (what, md, "direct", len(got[0]), len(want))
        assert np.array_equal(got[1], got[0]), (what, md)
L.check(lib.hvd_debug_set(b"allpairs_index", 1))
"""

_SIZE = _HEAD + """
assert W == {w}, W
check(planted({n}, seed={n}), {n})
print("SCATTER_OK", {n})
"""

_CONSTANT_BYTES = _HEAD + """
n = {n}
db = planted(n, seed=7000 + {seed})
for byte in {bytes}:
    db[:, byte] = 0xC3  # little-endian: an odd byte is the high byte of block byte >> 1
check(db, {bytes!r})
print("SCATTER_OK", n)
"""


def _child(code, seconds, devices=None):
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"} if devices else dict(os.environ)
    if devices:
        env["HVD_DEVICES"] = devices
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=seconds, text=True)
    assert r.returncode == 0 and "SCATTER_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("n", [2, 255, TILE - 1, TILE, TILE + 1, 2 * TILE + 17])
def test_sizes_around_a_tile(n):
    _child(_SIZE.format(root=ROOT, n=n, w=1), 240)


@pytest.mark.parametrize("which", ["block0", "block15", "every_block"])
def test_one_partition_takes_whole_tiles(which):
    odd = {"block0": (1,), "block15": (31,), "every_block": tuple(range(1, 32, 2))}[which]
    _child(_CONSTANT_BYTES.format(root=ROOT, n=TILE + 1 + 600, seed=len(odd) + odd[0], bytes=odd), 240)


def test_three_tiles_from_two_contexts_on_one_device():
    _child(_SIZE.format(root=ROOT, n=2 * TILE + 17, w=2), 240, devices="0,0")
