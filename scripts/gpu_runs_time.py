"""Times of the static-scene filter on one MI355X: HIP events on the library stream around the call, 3 warm-up
runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_runs_time.py [--reps 15] [--videos 50000] [--held-videos 50000] [--max-dist 8] > runs_time.jsonl
Two libraries:
  cfg5   the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the device)
  held   the first --held-videos videos of it with every frame held 1..8 times (the hold lengths drawn per frame, seed 7):
         what a library of slides, lectures or frame-rate conversions looks like to the rule
Legs, per library:
  frame_runs        hvd_dev_frame_runs alone (keep and run words; 32 B read and 8 B written per frame)
  without_repeated  the whole DeviceLibrary.without_repeated_frames step: rule, compaction, positions, gather of the run words
  match_raw / match_collapsed   DeviceLibrary.match_videos before and after the collapse, same process, same run
and a summary line: kept / raw frames, rule / step, step / search, collapsed / raw search next to (kept / raw)^2.
Prints one JSON line per leg."""
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
ap.add_argument("--max-dist", type=int, default=8)
args = ap.parse_args()
lib = L.init(0)
WARMUP = 3


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
    rec = dict(leg=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=args.reps, warmup=WARMUP, **extra)
    print(json.dumps(rec), flush=True)
    return rec


def legs(prefix, library):
    n, V = library.n_frames, library.n_videos
    d_keep, d_run = L.DeviceBuffer(4 * n), L.DeviceBuffer(4 * n)
    rule = leg(prefix + "frame_runs", lambda: L.check(lib.hvd_dev_frame_runs(
        library.d_hashes.ptr, library.d_offsets.ptr, V, n, args.max_dist, 0, d_keep.ptr, d_run.ptr)), frames=n, videos=V,
        max_dist=args.max_dist, bytes_per_frame=40)
    rule["gb_per_s"] = 40 * n / rule["ms_median"] / 1e6
    d_keep.free()
    d_run.free()

    def step():
        collapsed, _, d_runs = library.without_repeated_frames(args.max_dist)
        d_runs.free()
        collapsed.free()

    whole = leg(prefix + "without_repeated", step, frames=n)
    collapsed, dropped, d_runs = library.without_repeated_frames(args.max_dist)
    d_runs.free()
    library.image()
    collapsed.image()
    raw = leg(prefix + "match_raw", lambda: library.match_videos(), frames=n, records=len(library.match_videos()))
    after = leg(prefix + "match_collapsed", lambda: collapsed.match_videos(), frames=collapsed.n_frames,
                records=len(collapsed.match_videos()))
    share = collapsed.n_frames / max(n, 1)
    print(json.dumps(dict(leg=prefix + "summary", raw_frames=n, kept_frames=collapsed.n_frames, kept_over_raw=share,
                          rule_gb_per_s=rule["gb_per_s"], rule_over_step=rule["ms_median"] / whole["ms_median"],
                          step_over_raw_search=whole["ms_median"] / raw["ms_median"],
                          collapsed_over_raw_search=after["ms_median"] / raw["ms_median"], kept_over_raw_squared=share * share)),
          flush=True)
    collapsed.free()


# ---- the config-5 library ----
V, F = args.videos, 64
n = V * F
d_frames = L.DeviceBuffer(n * 4096)
L.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, 0, V, F, 5, None))
d_h, d_q = pipeline.hash_frames_on_device(d_frames.ptr, n, 64, 64, 1)
library = pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, n, np.arange(V + 1, dtype=np.int64) * F)
for b in (d_frames, d_h, d_q):
    b.free()
legs("cfg5_", library)

# ---- its held-frame variant: every frame of the first --held-videos videos held 1..8 times ----
offsets = library.offsets()[: min(args.held_videos, V) + 1]
hashes = library.hashes()[: offsets[-1]]
library.free()
hold = np.random.default_rng(7).integers(1, 9, len(hashes))
before = np.concatenate([[0], np.cumsum(hold)])
held = pipeline.DeviceLibrary.from_host(np.repeat(hashes, hold, axis=0), before[offsets].astype(np.int64))
legs("held_", held)
held.free()
