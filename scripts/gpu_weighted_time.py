"""Times of the duration-weighted video search on one MI355X: HIP events on the library stream around the call, 3
warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_weighted_time.py [--reps 15] [--videos 50000] [--held-videos 50000] [--out profiles/weighted_time.jsonl]
The library is the held-frame config-5 library of scripts/gpu_runs_time.py (--videos x 64 synthetic 64x64 frames, hashed and
filtered on the device, every frame of the first --held-videos videos held 1..8 times, seed 7), collapsed at max_dist 0 with the
runs attached as weights. Legs:
  match_collapsed   DeviceLibrary.match_videos on the collapsed library: the plain code path, the yardstick
  match_weighted    the same library, match_videos(weighted=True): the same compare and key set, the weighted fold
  video_weights     hvd_dev_video_weights alone (4 B read per frame, 8 B written per video)
and an identity line: whether match_weighted's records equal those of the plain search of the library BEFORE the collapse (one
run of it, timed once for scale), and whether the weight totals equal its lengths.
Prints one JSON line per leg and appends the same lines to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L, pipeline  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=50000)
ap.add_argument("--held-videos", type=int, default=50000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_time.jsonl"))
args = ap.parse_args()
lib = L.init(0)
WARMUP = 3


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    return rec


def timed(fn):
    L.check(lib.hvd_timer_start())
    fn()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    return float(ms.value)


def leg(name, fn, **extra):
    for _ in range(WARMUP):
        fn()
    ms = [timed(fn) for _ in range(args.reps)]
    return emit(dict(leg=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=args.reps, warmup=WARMUP, **extra))


# ---- the held-frame config-5 library ----
V, F = args.videos, 64
n = V * F
d_frames = L.DeviceBuffer(n * 4096)
L.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, 0, V, F, 5, None))
d_h, d_q = pipeline.hash_frames_on_device(d_frames.ptr, n, 64, 64, 1)
library = pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, n, np.arange(V + 1, dtype=np.int64) * F)
for b in (d_frames, d_h, d_q):
    b.free()
offsets = library.offsets()[: min(args.held_videos, V) + 1]
hashes = library.hashes()[: offsets[-1]]
library.free()
hold = np.random.default_rng(7).integers(1, 9, len(hashes))
before = np.concatenate([[0], np.cumsum(hold)])
held = pipeline.DeviceLibrary.from_host(np.repeat(hashes, hold, axis=0), before[offsets].astype(np.int64))

# ---- collapsed at max_dist 0, the runs attached ----
collapsed, dropped, d_runs = held.without_repeated_frames(0)
collapsed.attach_weights(d_runs)
collapsed.image()
kept, videos = collapsed.n_frames, collapsed.n_videos
plain = leg("match_collapsed", lambda: collapsed.match_videos(), frames=kept, videos=videos, records=len(collapsed.match_videos()))
weighted_records = collapsed.match_videos(weighted=True)
weighted = leg("match_weighted", lambda: collapsed.match_videos(weighted=True), frames=kept, videos=videos,
               records=len(weighted_records))
d_totals = L.DeviceBuffer(8 * max(videos, 1))
totals = leg("video_weights", lambda: L.check(lib.hvd_dev_video_weights(collapsed.d_weights.ptr, collapsed.d_offsets.ptr, videos, kept,
                                                                         0, d_totals.ptr)), frames=kept, videos=videos)
totals["gb_per_s"] = (4 * kept + 8 * videos) / totals["ms_median"] / 1e6
d_totals.free()

# ---- the identity at full size: one plain search of the library before the collapse ----
held.image()
raw_records = []
raw_ms = timed(lambda: raw_records.append(held.match_videos()))
spread = plain["ms_max"] - plain["ms_min"]
emit(dict(leg="summary", raw_frames=held.n_frames, kept_frames=kept, kept_over_raw=kept / max(held.n_frames, 1),
          match_raw_ms_once=raw_ms, records_equal_raw=bool(np.array_equal(weighted_records, raw_records[0])),
          totals_equal_raw_lengths=bool(np.array_equal(collapsed.weight_totals(), held.lengths())),
          weighted_over_plain=weighted["ms_median"] / plain["ms_median"],
          weighted_median_inside_plain_range=bool(plain["ms_min"] <= weighted["ms_median"] <= plain["ms_max"]),
          weighted_median_above_plain_max_by_more_than_its_spread=bool(weighted["ms_median"] > plain["ms_max"] + spread),
          video_weights_gb_per_s=totals["gb_per_s"]))
collapsed.free()
held.free()
