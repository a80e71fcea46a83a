"""Call times of the all-pairs pass with the pigeonhole index forced on one MI355X, on the two DBs that bound the
join: 1 M uniform hashes (the headline: many short work items) and 200 000 hashes with 5 000 rows in one bucket of block 0
(one wave walks that bucket alone: the longest work item, the rule's ps_crit). Host clock around `hvd.allpairs_hamming`
(host DB in, sorted pair list out: the copies are inside), 3 warm-ups, then the median of --reps calls with min..max.
  python scripts/gpu_index_join_time.py [--reps 10] [--label NAME]
Two builds are compared by running it once per build through HVD_LIB_PATH, in turn. Prints one JSON line per DB; `walk` is
the longest work item as the statistics kernel counts it, c_u x (c_u + the counts of the one-bit neighbours above u)."""
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


def get(key):
    v = C.c_int(0)
    L.check(lib.hvd_debug_get(key, C.byref(v)))
    return v.value


def longest_walk(db):
    """max over (b, u) of c_u x (c_u + the counts of the neighbours above u), as k_index_stats has it."""
    keys = np.ascontiguousarray(db).view("<u2").astype(np.int64)
    best = 0
    for b in range(16):
        cnt = np.bincount(keys[:, b], minlength=65536)
        u = np.arange(65536)
        ylen = cnt.copy()
        for t in range(16):
            above = ((u >> t) & 1) == 0
            ylen[above] += cnt[u[above] ^ (1 << t)]
        best = max(best, int((cnt * ylen).max()))
    return best


uniform, _ = synth.hash_db(1_000_000, seed=3)
crowded, _ = synth.hash_db(200_000, seed=5)
crowded[np.random.default_rng(5).choice(200_000, size=5000, replace=False), 0:2] = 0x5A
L.check(lib.hvd_debug_set(b"allpairs_index", 1))
for name, db in (("uniform_1m", uniform), ("crowded_200k_5000_in_one_bucket", crowded)):
    times, pairs = [], None
    for rep in range(3 + args.reps):
        t = time.perf_counter()
        got = hvd.allpairs_hamming(db, 31)
        dt = (time.perf_counter() - t) * 1e3
        assert get(b"allpairs_index_used") == 1
        assert pairs is None or len(got) == pairs
        pairs = len(got)
        if rep >= 3:
            times.append(dt)
    print(json.dumps({"build": args.label, "db": name, "hashes": len(db), "max_dist": 31, "index": "forced",
                      "what": "hvd.allpairs_hamming call time, host clock, copies inside", "median_ms": round(statistics.median(times), 4),
                      "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "reps": len(times), "pairs": pairs,
                      "kcand": get(b"allpairs_index_kcand"), "walk": longest_walk(db)}), flush=True)
L.check(lib.hvd_debug_set(b"allpairs_index", -1))
