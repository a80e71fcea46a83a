"""The config-5 library (50 000 videos x 64 gray 64x64 frames from hvd_dev_synth_video_frames, 2 % copies) through the
chained device pipeline: plain (dedupe_frames_on_device), "mirror" and "dihedral" (dedupe_transformed_frames_on_device).
Legs interleaved, one warm-up round, median of REPS rounds of host wall time with the stage split the pipeline reports;
then the dihedral compaction alone (hvd_dev_compact_kept_dihedral, HIP events) with the bytes its kernels must move over
that time. env: V (50000), REPS (5), OUT (json path, optional)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hvd_amd import _lib as L, pipeline as P, search  # noqa: E402

lib = L.init(0)
V, F = int(os.environ.get("V", 50000)), 64
REPS = int(os.environ.get("REPS", 5))
n = V * F
rng = np.random.default_rng(5)
copy_of = np.full(V, -1, np.int32)
dst = rng.choice(np.arange(1, V), size=V // 50, replace=False)
is_dst = np.zeros(V, bool)
is_dst[dst] = True
copy_of[dst] = rng.choice(np.flatnonzero(~is_dst), size=dst.size)
d_copy = L.DeviceBuffer.from_array(copy_of)
d_fr = L.DeviceBuffer(n * 4096)
L.check(lib.hvd_dev_synth_video_frames(d_fr.ptr, 0, V, F, 5, d_copy.ptr))
L.check(lib.hvd_dev_sync())
raw_off = np.arange(V + 1, dtype=np.int64) * F


def leg(name):
    tm = {}
    t0 = time.perf_counter()
    if name == "plain":
        pairs = P.dedupe_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1, timings=tm)[0]
        tm["cross_ms"] = 0.0
    else:
        pairs = P.dedupe_transformed_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1, transforms=name, timings=tm)[0]
    tm["total_ms"] = (time.perf_counter() - t0) * 1e3
    tm["pairs"] = len(pairs)
    return tm


LEGS = ("plain", "mirror", "dihedral")
for name in LEGS:  # warm-up: code objects, record buffers, scratch pools
    leg(name)
runs = {name: [] for name in LEGS}
for _ in range(REPS):
    for name in LEGS:
        runs[name].append(leg(name))
KEYS = ("total_ms", "hash_ms", "compact_ms", "search_ms", "cross_ms")
out = {"V": V, "F": F, "reps": REPS, "legs": {}}
for name in LEGS:
    out["legs"][name] = {k: float(np.median([r[k] for r in runs[name]])) for k in KEYS}
    out["legs"][name]["pairs"] = runs[name][0]["pairs"]
base = out["legs"]["plain"]["total_ms"]
for name in LEGS:
    out["legs"][name]["ratio"] = out["legs"][name]["total_ms"] / base

# the compaction alone, on the dihedral hashes of the whole library
d_h8, d_q = P.hash_frames_dihedral_on_device(d_fr.ptr, n, 64, 64, 1)
kept_q = int((d_q.to_array(np.int32, n) >= 31).sum())
d_roff = L.DeviceBuffer.from_array(raw_off)
bufs = [L.DeviceBuffer(b) for b in (32 * n, 8 * (V + 1), 4 * n, 7 * 32 * n, 7 * 4 * n, 7 * 4 * n)]
out["compaction"] = {}
for name in ("mirror", "flips", "dihedral"):
    names = search.transform_set(name)
    S, K = len(names), len(names) - 1
    kept = C.c_int64(0)
    ms = []
    for rep in range(REPS + 1):
        L.check(lib.hvd_timer_start())
        L.check(lib.hvd_dev_compact_kept_dihedral(d_h8.ptr, d_q.ptr, n, d_roff.ptr, V, 31, P.transform_mask(names),
                                                  *[b.ptr for b in bufs], C.byref(kept)))
        t = C.c_float(0)
        L.check(lib.hvd_timer_stop(C.byref(t)))
        if rep:
            ms.append(t.value)
    k = kept.value
    assert k == kept_q
    # bytes the four kernels must move: quality read 3 x 4n, positions 4n written + read, frame -> video 4k written +
    # read, the selected variants of the kept frames 32kS read + written, query video / exclusion id 8kK, offsets ~3 x 8V
    nbytes = 12 * n + 8 * n + 8 * k + 64 * k * S + 8 * k * K + 24 * (V + 1)
    med = float(np.median(ms))
    out["compaction"][name] = {"ms": med, "kept": k, "bytes": nbytes, "GB_per_s": nbytes / med / 1e6,
                               "share_of_6.3TB_per_s": nbytes / med / 1e6 / 6300.0}
for b in bufs + [d_h8, d_q, d_roff, d_fr, d_copy]:
    b.free()
print(json.dumps(out, indent=1))
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        json.dump(out, f, indent=1)
