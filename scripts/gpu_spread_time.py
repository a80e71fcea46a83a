"""Times of the common-frame filter on one MI355X beside the search it borrows its compare from: HIP events on
the library stream around each call, one warm-up run of each, then --reps runs, the two searches alternating, all in one
process.
  python scripts/gpu_spread_time.py [--reps 9] [--hashes 1000000] > spread_time.jsonl
The library is the benchmark's clustered one: --hashes frame hashes with 10^4 clusters of 10 near-identical ones, grouped into
videos of 64 frames. Legs:
  match_videos   DeviceLibrary.match_videos(): compare, key set, fold into the pair map, emit, read-back of the records
  spread         DeviceLibrary.spread(): the same compare and key set, then k_keys_to_spread instead of the fold
  rule           hvd_dev_common_frames alone (k_common_rule), max_videos 5, max_share 50
  gather         hvd_dev_gather_kept_i32 alone (k_keep_count, k_scan_block_sums, k_gather_kept_i32)
  filter         DeviceLibrary.without_common_frames(5, 50): spread, rule, compaction, positions
Prints one JSON line per leg (median, min, max in ms) and one with what was computed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L, synth  # noqa: E402
from hvd_amd.pipeline import DeviceLibrary  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--hashes", type=int, default=1_000_000)
args = ap.parse_args()
lib = L.init(0)
n = args.hashes - args.hashes % 64
db, _ = synth.hash_db_clustered(n, 10_000, 10, seed=8)
library = DeviceLibrary.from_host(db, np.arange(0, n + 1, 64, dtype=np.int64))
library.image()


def timed(fn):
    L.check(lib.hvd_timer_start())
    out = fn()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    return float(ms.value), out


def spread_once():
    library.spread().free()


def leg(name, times):
    print(json.dumps({"leg": name, "ms": round(statistics.median(times), 4), "min": round(min(times), 4),
                      "max": round(max(times), 4), "reps": len(times)}), flush=True)


records = library.match_videos()
spread_once()
match, spread = [], []
for _ in range(args.reps):
    match.append(timed(library.match_videos)[0])
    spread.append(timed(spread_once)[0])
leg("match_videos", match)
leg("spread", spread)
d_spread = library.spread()
d_keep, d_out = L.DeviceBuffer(4 * n), L.DeviceBuffer(4 * n)


def rule():
    L.check(lib.hvd_dev_common_frames(d_spread.ptr, library.d_offsets.ptr, library.n_videos, n, 5, 50, d_keep.ptr))


def gather():
    L.check(lib.hvd_dev_gather_kept_i32(d_spread.ptr, d_keep.ptr, n, d_out.ptr))


rule()
gather()
leg("rule", [timed(rule)[0] for _ in range(args.reps)])
leg("gather", [timed(gather)[0] for _ in range(args.reps)])
times, dropped = [], None
for _ in range(1 + args.reps):
    ms, (filtered, dropped) = timed(lambda: library.without_common_frames(5, 50))
    filtered.free()
    times.append(ms)
leg("filter", times[1:])
host_spread = d_spread.to_array(np.int32, n)
print(json.dumps({"hashes": n, "videos": library.n_videos, "records": int(len(records)), "keys": int(host_spread.sum(dtype=np.int64)),
                  "spread_max": int(host_spread.max()), "dropped_at_5_50": int(dropped.sum())}))
