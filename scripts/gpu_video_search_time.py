"""The video-search legs of bench.py --full, alone and repeated: usage gpu_video_search_time.py [TREE [LABEL]]. One JSON line.
TREE: the checkout whose package and library are timed (default: this one), so that two builds can alternate in one session.
video_match: bench.py's K3 leg (2000 videos x 64 frame hashes, host buffers in, records out), its cross and weighted forms and
the host spread on the same library. device_match_videos: config 5's device-resident search (50 000 videos x 64 frames hashed
and compacted in HBM, DeviceLibrary.match_videos)."""
import json
import os
import sys
import time

import numpy as np

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
label = sys.argv[2] if len(sys.argv) > 2 else "this tree"
sys.path.insert(0, tree)
import hvd_amd  # noqa: E402
from hvd_amd import _lib as L, pipeline, search, synth  # noqa: E402

assert os.path.dirname(os.path.abspath(hvd_amd.__file__)) == tree, hvd_amd.__file__
lib = L.init(0)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        L.check(lib.hvd_device_synchronize())
        t = time.perf_counter()
        r = fn()
        out.append(1e3 * (time.perf_counter() - t))
    return r, out


def stats(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


res = {"label": label, "lib": L.LIB_PATH}
vfr, voff, _ = synth.video_hashes(2000, seed=7, frames_per_video=64, copy_fraction=0.02)
search.match_videos(vfr[:6400], voff[:101])  # warm
rec, ms = timed(lambda: search.match_videos(vfr, voff), 9)
res["video_match"] = dict(stats(ms), records=int(len(rec)))
half = 1000
fq, oq = vfr[: half * 64], voff[: half + 1]
ft, ot = vfr[half * 64:], voff[half:] - voff[half]
rec, ms = timed(lambda: search.match_videos_cross(fq, oq, ft, ot), 9)
res["video_match_cross"] = dict(stats(ms), records=int(len(rec)))
ones = np.ones(len(vfr), np.int32)
rec, ms = timed(lambda: search.match_videos(vfr, voff, weights=ones), 9)
res["video_match_weighted"] = dict(stats(ms), records=int(len(rec)))
_, ms = timed(lambda: search.frame_spread(vfr, voff), 9)
res["frame_spread"] = stats(ms)

V, F = 50000, 64
n = V * F
d_frames = L.DeviceBuffer(n * 4096)
L.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, 0, V, F, 5, None))
L.check(lib.hvd_dev_sync())
raw_off = np.arange(V + 1, dtype=np.int64) * F
d_h, d_q = pipeline.hash_frames_on_device(d_frames.ptr, n, 64, 64, 1)
libr = pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, n, raw_off)
libr.image()
libr.match_videos()  # warm
rec, ms = timed(lambda: libr.match_videos(), 7)
res["device_match_videos"] = dict(stats(ms), records=int(len(rec)), kept=libr.n_frames)
for buf in (d_h, d_q, libr, d_frames):
    buf.free()
print(json.dumps(res), flush=True)
