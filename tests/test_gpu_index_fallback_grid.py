"""The matrix-core fall-back of a pass that was eligible for the index, on the coarse grid it is launched with behind an index
launch (csrc/k_hamming_mfma.hip: launch_auto; csrc/hvd_mfma_forms.h: kSelfCapBehindIndex). n = 300 000 is the smallest round
size at which that geometry differs from every other self pass's for all three forms: chunks of 10 752 columns x 28 (forms 9,
18) and 21 504 x 14 (form 12) instead of 8 192 x 37 (tests/test_mfma_geometry_behind_index.py). Auto mode (-1) is compared
with the index switched off (0: the knob's geometry) on the same DB: equal pair lists, a few thousand planted pairs at
distances 0 .. 40 among them, and the index used in neither. Two DBs, both with 5 % of the rows in one bucket of block 0, so
that the statistics refuse the index (the longest walk is 15 000 x 15 000 = 2.25e8 pairs, priced at 72 ms against a matrix-
core pass of 1.8 ms): uniform random hashes, on which the probe chooses form 9, and a dense DB -- 300 prototypes, every row
one of them with about 40 random flips, so that the first 128 bits of two rows of one prototype often agree within the
tolerance -- on which it chooses form 18 or 12. One more case runs the uniform DB as two contexts on one device, so that the
rank arithmetic sees the coarse chunk. Every GPU step is a child process of its own under a time limit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_HEAD = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np, hvd_amd
from hvd_amd import _lib as L
lib = L.ensure()
def mode(m): L.check(lib.hvd_debug_set(b"allpairs_index", m))
def get(key):
    v = C.c_int(0); L.check(lib.hvd_debug_get(key, C.byref(v))); return v.value
def flip(rng, row, k):
    out = np.unpackbits(row.copy()); out[rng.choice(256, size=k, replace=False)] ^= 1
    return np.packbits(out)
N = 300000
def finish(db, rng):
    for j, k in enumerate(range(0, N - 1, 40)):
        db[k + 1] = flip(rng, db[k], j % 41)  # 7500 near-duplicates at distances 0 .. 40
    db[: N // 20, 0:2] = (0x11, 0xC3)  # 5 % of the rows in one bucket of block 0
    return db
def uniform(seed):
    rng = np.random.default_rng(seed)
    return finish(rng.integers(0, 256, (N, 32), dtype=np.uint8), rng)
def dense(seed):
    rng = np.random.default_rng(seed)
    protos = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    bits = np.unpackbits(protos[rng.integers(0, 300, N)], axis=1)
    bits[np.arange(N)[:, None], rng.integers(0, 256, (N, 40))] ^= 1  # about 40 flips each (a position drawn twice flips once)
    return finish(np.packbits(bits, axis=1), rng)
def both_modes(db, contexts=1):
    out = []
    for m in (0, -1):
        mode(m)
        got = hvd_amd.allpairs_hamming(db, 31)
        for k in range(contexts):
            if contexts > 1: L.set_context(k)
            assert get(b"allpairs_index_used") == 0, (m, k)
        if contexts > 1: L.set_context(0)
        out.append(got)
    ref, got = out
    assert len(np.unique(got[["i", "j"]])) == len(got)
    assert 4000 < len(ref) and np.array_equal(got, ref), (len(got), len(ref))
    assert (ref["dist"] == 0).any() and (ref["dist"] == 31).any()
    return get(b"mfma_auto_form")
"""

_FORMS = _HEAD + """
f_uniform = both_modes(uniform(31))
f_dense = both_modes(dense(32))
assert f_uniform == 9 and f_dense in (12, 18), (f_uniform, f_dense)
print("FALLBACK_OK", f_uniform, f_dense)
"""

_TWO_CONTEXTS = _HEAD + """
W = L.context_count(); assert W == 2, W
print("FALLBACK_OK", both_modes(uniform(33), contexts=W))
"""


def _child(code, seconds, devices=None):
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"} if devices else dict(os.environ)
    if devices:
        env["HVD_DEVICES"] = devices
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=seconds, text=True)
    assert r.returncode == 0 and "FALLBACK_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


def test_fallback_equals_the_pass_without_index_on_form_9_and_another():
    _child(_FORMS.format(root=ROOT), 300)


def test_two_contexts_on_one_device():
    _child(_TWO_CONTEXTS.format(root=ROOT), 300, devices="0,0")
