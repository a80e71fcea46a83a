"""Times of the filtered ingest on one MI355X beside the route that gives the same answer without it: a host
clock that ends in hvd_dev_sync around each route, one warm-up run of each, then --reps runs, the two routes alternating, all
in one process.
  python scripts/gpu_ingest_time.py [--reps 9] [--hashes 1000000] [--new-videos 1000] [--max-videos 5] > ingest_time.jsonl
The library is the benchmark's clustered one: --hashes frame hashes with 10^4 clusters of 10 near-identical ones, grouped into
videos of 64. T is all but the last --new-videos videos, resident with its spread attached; Q is the last --new-videos. Routes:
  ingest         T.ingest(Q, M, 50), M = --max-videos: union, spread of Q, one cross spread on top of the attached one, rule,
                 two compactions, new x old and new x new searches, read-back of the records
  full           U.without_common_frames(M, 50), then match_videos() of the result, U = T || Q resident: the spread, the
                 rule, the compaction and the search over the whole union
Their records with a new video must be equal, or the script stops before it prints a time -- at M and at --check-videos
(default 9: every frame of this library is in at most 9 other videos, so nothing is dropped and the records are those of
the plain search; at 5 every clustered frame is dropped and no record is left). Then the legs of the ingest, each
timed alone the same way (--reps runs after one warm-up):
  extended       T.extended(Q)
  spread_new     Q.spread()
  spread_cross   T.spread_cross(Q): compare and key set of the rectangle, then k_keys_to_spread_cross
  match_library  T.match_library(Q): the same rectangle with the fold, the emit and the read-back
  match_new      Q.match_videos()
Prints one JSON line per route and leg (median, min, max in ms) and one with what was computed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L, synth  # noqa: E402
from hvd_amd.pipeline import DeviceLibrary  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--hashes", type=int, default=1_000_000)
ap.add_argument("--new-videos", type=int, default=1000)
ap.add_argument("--max-videos", type=int, default=5)
ap.add_argument("--check-videos", type=int, default=9)
args = ap.parse_args()
lib = L.init(0)
n = args.hashes - args.hashes % 64
V = n // 64
VT = V - args.new_videos
db, _ = synth.hash_db_clustered(n, 10_000, 10, seed=8)
old = DeviceLibrary.from_host(db[:64 * VT], np.arange(0, 64 * VT + 1, 64, dtype=np.int64))
new = DeviceLibrary.from_host(db[64 * VT:], np.arange(0, n - 64 * VT + 1, 64, dtype=np.int64))
whole = DeviceLibrary.from_host(db, np.arange(0, n + 1, 64, dtype=np.int64))
for library in (old, new, whole):
    library.image()
old.attach_spread()


def timed(fn):
    L.check(lib.hvd_dev_sync())
    t0 = time.perf_counter()
    out = fn()
    L.check(lib.hvd_dev_sync())
    return (time.perf_counter() - t0) * 1e3, out


def ingest(max_videos=args.max_videos):
    got = old.ingest(new, max_videos, 50)
    got.library.free()
    return got


def full(max_videos=args.max_videos):
    filtered, dropped = whole.without_common_frames(max_videos, 50)
    try:
        return filtered.match_videos(), dropped
    finally:
        filtered.free()


def leg(name, times):
    print(json.dumps({"leg": name, "ms": round(statistics.median(times), 4), "min": round(min(times), 4),
                      "max": round(max(times), 4), "reps": len(times)}), flush=True)


def free_all(buffers):
    for b in buffers:
        b.free()


checked = {}
for max_videos in (args.check_videos, args.max_videos):  # (the second pass is the warm-up of the timed routes)
    got = ingest(max_videos)
    records, dropped = full(max_videos)
    new_records = records[records["b"] >= VT]
    if not (np.array_equal(got.records, new_records) and np.array_equal(got.dropped, dropped)):
        sys.exit(f"the routes disagree at max_videos={max_videos}: {len(got.records)} records by the ingest, {len(new_records)} of "
                 f"{len(records)} by the full route: the timing is void")
    checked[max_videos] = int(len(new_records))
t_ingest, t_full = [], []
for _ in range(args.reps):
    t_ingest.append(timed(ingest)[0])
    t_full.append(timed(full)[0])
leg("ingest", t_ingest)
leg("full", t_full)
for name, fn in (("extended", lambda: old.extended(new).free()), ("spread_new", lambda: new.spread().free()),
                 ("spread_cross", lambda: free_all(old.spread_cross(new))), ("match_library", lambda: old.match_library(new)),
                 ("match_new", new.match_videos)):
    fn()
    leg(name, [timed(fn)[0] for _ in range(args.reps)])
print(json.dumps({"hashes": n, "videos": V, "library_videos": VT, "new_videos": V - VT, "new_frames": n - 64 * VT,
                  "max_videos": args.max_videos, "records_with_a_new_video": int(len(new_records)),
                  "records_of_the_union": int(len(records)), "dropped": int(dropped.sum()),
                  "equal_records_checked_at": checked, "ingest_over_full": round(statistics.median(t_ingest) /
                                                                                   statistics.median(t_full), 4)}))
