"""Call times of an all-pairs pass that was eligible for the pigeonhole index and falls back to the matrix cores
on one MI355X: what the coarse grid of the launches behind an index launch (csrc/hvd_mfma_forms.h: kSelfCapBehindIndex) costs
the pass that does run on them. Two DBs of 1 M hashes in auto mode, both with 5 % of the rows in one bucket of block 0, so that
the statistics refuse the index: uniform hashes (the crowded DB of profiles/r10_index_crowded.txt), and a pair-rich variant in
which the crowded rows are near-duplicates (20 flips each) of 300 prototypes -- a few hundred thousand pairs, packed into few
tiles, where a workgroup's pair buffer overflows first. Host clock around `hvd.allpairs_hamming` (host DB in, sorted pair
list out: the copies are inside), 3 warm-ups, then the median of --reps calls with min..max.
  python scripts/gpu_index_fallback_time.py [--reps 10] [--label NAME]
Two builds are compared by running it once per build through HVD_LIB_PATH, in turn. Prints one JSON line per DB."""
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
import hvd_amd as hvd  # noqa: E402
from hvd_amd import _lib as L, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--label", default=os.path.basename(L.LIB_PATH))
args = ap.parse_args()
lib = L.init(0)
N = 1_000_000


def get(key):
    v = C.c_int(0)
    L.check(lib.hvd_debug_get(key, C.byref(v)))
    return v.value


crowded, _ = synth.hash_db(N, seed=3)
crowded[: N // 20, 0:2] = 0x5A
rng = np.random.default_rng(7)
rich = crowded.copy()
bits = np.unpackbits(rng.integers(0, 256, (300, 32), dtype=np.uint8)[rng.integers(0, 300, N // 20)], axis=1)
bits[np.arange(N // 20)[:, None], rng.integers(0, 256, (N // 20, 20))] ^= 1
rich[: N // 20] = np.packbits(bits, axis=1)
rich[: N // 20, 0:2] = 0x5A
for name, db in (("crowded_1m_5pct_in_one_bucket", crowded), ("crowded_1m_pair_rich", rich)):
    times, pairs = [], None
    for rep in range(3 + args.reps):
        t = time.perf_counter()
        got = hvd.allpairs_hamming(db, 31, cap=1 << 22)
        dt = (time.perf_counter() - t) * 1e3
        assert get(b"allpairs_index_used") == 0
        assert pairs is None or len(got) == pairs
        pairs = len(got)
        if rep >= 3:
            times.append(dt)
    print(json.dumps({"build": args.label, "db": name, "hashes": len(db), "max_dist": 31, "index": "auto, refused",
                      "what": "hvd.allpairs_hamming call time, host clock, copies inside", "median_ms": round(statistics.median(times), 4),
                      "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "reps": len(times), "pairs": pairs,
                      "form": get(b"mfma_auto_form")}), flush=True)
