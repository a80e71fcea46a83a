"""Run by tests/test_gpu_autocrop.py in a process of its own with HVD_DEVICES=0,0 (the device group is process state): the
host entry of the content-rectangle hash under a group of two contexts, against the CPU oracle over the contiguous crops."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import autocrop_helpers as A  # noqa: E402
import hvd_amd  # noqa: E402
from hvd_amd import _lib as L  # noqa: E402
from oracle import oracle as O  # noqa: E402  (the checker)

O.build()
L.ensure()
assert L.context_count() == 2, L.context_count()
rng = np.random.default_rng(3)
vids, rects = [], []
for k, (b, ax) in enumerate(A.LAYOUTS):
    fr, rc = A.barred(k, b, ax, rng, nf=3)
    vids.append(fr)
    rects.append(rc)
vids.append(A.content(512, 512, 9, nf=2))
rects.append((0, 0, 512, 512))
frames = np.concatenate(vids)
off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
h, q, r = hvd_amd.vpdq.hash_frames_autocrop(frames, off)
assert r.tolist() == [list(x) for x in rects] and np.array_equal(r, A.rule_rects(frames, off))
wh, wq = A.oracle_cropped(O, frames, off, r)
assert np.array_equal(h, wh) and np.array_equal(q, wq)
for ctx in (1, 0):  # the call runs on the calling thread's current context: either gives the same bytes
    L.set_context(ctx)
    h2, q2, r2 = hvd_amd.vpdq.hash_frames_autocrop(frames, off)
    assert np.array_equal(h2, h) and np.array_equal(q2, q) and np.array_equal(r2, r)
print("AUTOCROP_GROUP_OK")
