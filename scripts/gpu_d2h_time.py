"""Call times of hvd_memcpy_d2h on one MI355X at the sizes around its small-copy threshold (csrc/hvd_internal.h: kSmallD2hMax;
DESIGN 4.1): 8 B (a pair count), 16 KB (the headline's records), 64 KB and 256 KB, from device memory into pageable host
memory. Host clock around the call (it ends in a stream synchronise), 100 warm-ups, then the median of --reps calls per size.
  python scripts/gpu_d2h_time.py [--reps 1000] [--label NAME]
Two builds are compared by running it once per build through HVD_LIB_PATH, in turn. Prints one JSON line per size."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--label", default=os.path.basename(L.LIB_PATH))
args = ap.parse_args()
lib = L.init(0)

SIZES = (8, 16 << 10, 64 << 10, 256 << 10)
data = np.random.default_rng(1).integers(0, 256, max(SIZES), dtype=np.uint8)
src = L.DeviceBuffer.from_array(data)
dst = np.zeros(max(SIZES), np.uint8)
d_ptr, h_ptr = C.c_void_p(src.ptr), C.c_void_p(dst.ctypes.data)
for nbytes in SIZES:
    n, times = C.c_size_t(nbytes), []
    for rep in range(100 + args.reps):
        t = time.perf_counter()
        rc = lib.hvd_memcpy_d2h(h_ptr, d_ptr, n)
        dt = (time.perf_counter() - t) * 1e6
        L.check(rc)
        if rep >= 100:
            times.append(dt)
    assert np.array_equal(dst[:nbytes], data[:nbytes])
    dst[:] = 0
    times.sort()
    print(json.dumps({"build": args.label, "bytes": nbytes, "what": "hvd_memcpy_d2h call time, host clock, pageable destination",
                      "median_us": round(statistics.median(times), 2), "p10_us": round(times[len(times) // 10], 2),
                      "p90_us": round(times[len(times) * 9 // 10], 2), "reps": len(times)}), flush=True)
src.free()
