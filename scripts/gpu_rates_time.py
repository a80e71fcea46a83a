"""Times of the rate-aware alignment on one MI355X, beside the single-offset call it extends: HIP events on the
library stream around the call, 3 warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_rates_time.py [--reps 15] [--videos 50000] > rates_time.jsonl
Legs:
  match_videos     the video search of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
                   device): the candidates, and the time the alignment is an addition to
  align            hvd_dev_vpdq_align_videos of every record of that search (index positions, slack 1): the baseline
  rates_r1 / _r8   hvd_dev_vpdq_align_rates of the same records under [(1, 1)] and under the eight default rates; the first
                   twelve words under [(1, 1)] are checked against the align records
  planted_align / planted_rates_r1 / _r8   4 096 pairs of a 60-frame clip at 5/4 against its 600-frame source
Every ratio is against the single-offset call of the same process. Prints one JSON line per leg."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L, pipeline, search, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=50000)
args = ap.parse_args()
lib = L.init(0)
WARMUP = 3
RATES = {1: ((1, 1),), 8: search.DEFAULT_RATES}


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


def calls(library, pairs, slack=1):
    """The buffers of the alignment calls over `library` against itself, and call(R): R = 0 the single-offset entry, else
    hvd_dev_vpdq_align_rates under RATES[R]. -> call, read(R) -> records, buffers."""
    M = len(pairs)
    span = int(library.lengths().max()) - 1
    bins = min(max((n + d) * span + 1 + 2 * slack * max(n, d) for n, d in RATES[8]), L.ALIGN_MAX_BINS)
    sb = C.c_size_t(0)
    L.check(lib.hvd_rates_scratch_bytes(bins, C.byref(sb)))  # (the same sizing rule as hvd_align_scratch_bytes, on more bins)
    d_pairs = L.DeviceBuffer.from_array(np.ascontiguousarray(pairs, dtype=np.uint32))
    d_out = L.DeviceBuffer(L.VRATE_DTYPE.itemsize * max(M, 1))
    d_scr = L.DeviceBuffer(sb.value) if sb.value else None
    h, o, V, scr = library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, d_scr.ptr if d_scr else None
    lists = {R: search.rate_array(r) for R, r in RATES.items()}

    def call(R):
        if R == 0:
            L.check(lib.hvd_dev_vpdq_align_videos(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, scr, sb.value, d_out.ptr))
        else:
            L.check(lib.hvd_dev_vpdq_align_rates(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, lists[R].ctypes.data,
                                                 len(lists[R]), scr, sb.value, d_out.ptr))

    def read(R):
        call(R)
        return d_out.to_array(L.VALIGN_DTYPE if R == 0 else L.VRATE_DTYPE, M)

    return call, read, (d_pairs, d_out, d_scr), bins


def three_legs(prefix, library, pairs, **extra):
    call, read, bufs, bins = calls(library, pairs)
    al, r1, r8 = read(0), read(1), read(8)
    for f in L.VALIGN_DTYPE.names:
        assert np.array_equal(r1[f], al[f]), f
    assert (r8["band_votes"] >= al["band_votes"]).all()
    won = np.bincount(r8["rate_index"][r8["q_hits"] > 0], minlength=8).tolist()
    out = [leg(prefix + "align", lambda: call(0), pairs=len(pairs), **extra),
           leg(prefix + "rates_r1", lambda: call(1), pairs=len(pairs), matrix_passes_per_pair=2),
           leg(prefix + "rates_r8", lambda: call(8), pairs=len(pairs), matrix_passes_per_pair=9, largest_bins=bins,
               pairs_by_winning_rate=won, aligned_frames_r8=int(r8["q_aligned"].sum()), aligned_frames_align=int(al["q_aligned"].sum()))]
    for b in bufs:
        if b is not None:
            b.free()
    return out


# ---- the config-5 library ----
V, F = args.videos, 64
n = V * F
d_frames = L.DeviceBuffer(n * 4096)
L.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, 0, V, F, 5, None))
d_h, d_q = pipeline.hash_frames_on_device(d_frames.ptr, n, 64, 64, 1)
library = pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, n, np.arange(V + 1, dtype=np.int64) * F)
for b in (d_frames, d_h, d_q):
    b.free()
library.image()
recs = library.match_videos()
found = leg("match_videos", lambda: library.match_videos(), videos=V, kept_frames=library.n_frames, records=len(recs))
al, r1, r8 = three_legs("", library, np.stack([recs["a"], recs["b"]], axis=1))
print(json.dumps(dict(leg="summary", r1_over_align=r1["ms_median"] / al["ms_median"], r8_over_align=r8["ms_median"] / al["ms_median"],
                      expected_passes_9_over_2=4.5, r8_over_search=r8["ms_median"] / found["ms_median"])), flush=True)
library.free()

# ---- pairs that really are resampled: a 60-frame clip at 5/4 of a 600-frame source ----
rng = np.random.default_rng(7)
source = synth.hash_db(600, seed=7, plant_fraction=0.0)[0]
clip = source[np.floor(np.arange(60) * 5 / 4 + 100.3 + 0.5).astype(np.int64)]
clip = synth.flip_bits(clip, rng.integers(0, 25, 60), rng)
clip_lib = pipeline.DeviceLibrary.from_host(np.concatenate([clip, source]), np.array([0, 60, 660], dtype=np.int64))
al, r1, r8 = three_legs("planted_", clip_lib, np.tile(np.array([[0, 1]]), (4096, 1)), frames="60 x 600 at 5/4")
print(json.dumps(dict(leg="planted_summary", r1_over_align=r1["ms_median"] / al["ms_median"],
                      r8_over_align=r8["ms_median"] / al["ms_median"], expected_passes_9_over_2=4.5)), flush=True)
clip_lib.free()
