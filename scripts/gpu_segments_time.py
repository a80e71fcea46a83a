"""Times of the multi-segment alignment on one MI355X, beside the single-offset call it extends: HIP events on the
library stream around the call, 3 warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_segments_time.py [--reps 15] [--videos 50000] > segments_time.jsonl
Legs:
  match_videos     the video search of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
                   device): the candidates, and the time the alignment is an addition to
  align            hvd_dev_vpdq_align_videos of every record of that search (index positions, slack 1): the existing call
  segments_k1/_k8  hvd_dev_vpdq_align_segments of the same records at max_segments 1 and 8 (min_band_votes 1); seg[0] is checked
                   against the align records
  reel_align / reel_segments_k8   4 096 pairs of a 60-frame reel of 5 x 12 frames against its 600-frame source: a pair that
                   really has 5 segments costs 11 passes against 2
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
from hvd_amd import _lib as L, pipeline, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=50000)
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


def calls(library, pairs, slack=1):
    """The buffers of the alignment calls over `library` against itself, and call(K): K = 0 the single-offset entry, else
    hvd_dev_vpdq_align_segments at max_segments K. -> call, read(K) -> records, buffers."""
    M = len(pairs)
    bins = min(2 * int(library.lengths().max()) - 1 + 2 * slack, L.ALIGN_MAX_BINS)
    sb = C.c_size_t(0)
    L.check(lib.hvd_segments_scratch_bytes(bins, C.byref(sb)))  # (never smaller than hvd_align_scratch_bytes)
    d_pairs = L.DeviceBuffer.from_array(np.ascontiguousarray(pairs, dtype=np.uint32))
    d_out = L.DeviceBuffer(L.VSEGMENTS_DTYPE.itemsize * max(M, 1))
    d_scr = L.DeviceBuffer(sb.value) if sb.value else None
    h, o, V, scr = library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, d_scr.ptr if d_scr else None

    def call(K):
        if K == 0:
            L.check(lib.hvd_dev_vpdq_align_videos(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, scr, sb.value, d_out.ptr))
        else:
            L.check(lib.hvd_dev_vpdq_align_segments(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, K, 1, scr, sb.value,
                                                    d_out.ptr))

    def read(K):
        call(K)
        return d_out.to_array(L.VALIGN_DTYPE if K == 0 else L.VSEGMENTS_DTYPE, M)

    return call, read, (d_pairs, d_out, d_scr)


def three_legs(prefix, library, pairs, **extra):
    call, read, bufs = calls(library, pairs)
    al, s1, s8 = read(0), read(1), read(8)
    for f in L.VSEGMENT_DTYPE.names:
        assert np.array_equal(s1["seg"][f][:, 0], al[f]) and np.array_equal(s8["seg"][f][:, 0], al[f]), f
    hist = np.bincount(s8["n_segments"], minlength=9).tolist()
    out = [leg(prefix + "align", lambda: call(0), pairs=len(pairs), **extra),
           leg(prefix + "segments_k1", lambda: call(1), pairs=len(pairs)),
           leg(prefix + "segments_k8", lambda: call(8), pairs=len(pairs), pairs_by_n_segments=hist,
               matrix_passes=int((2 * s8["n_segments"] + ((s8["n_segments"] < 8) & (s8["q_covered"] < library.lengths()[s8["a"]])
                                                          & (s8["t_covered"] < library.lengths()[s8["b"]]))).sum()))]
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
search = leg("match_videos", lambda: library.match_videos(), videos=V, kept_frames=library.n_frames, records=len(recs))
al, s1, s8 = three_legs("", library, np.stack([recs["a"], recs["b"]], axis=1))
print(json.dumps(dict(leg="summary", k1_over_align=s1["ms_median"] / al["ms_median"], k8_over_align=s8["ms_median"] / al["ms_median"],
                      k8_over_search=s8["ms_median"] / search["ms_median"])), flush=True)
library.free()

# ---- pairs that really have five segments ----
rng = np.random.default_rng(7)
source = synth.hash_db(600, seed=7, plant_fraction=0.0)[0]
reel = np.concatenate([source[s:s + 12] for s in (40, 410, 130, 520, 255)])
reel = synth.flip_bits(reel, rng.integers(0, 25, 60), rng)
reel_lib = pipeline.DeviceLibrary.from_host(np.concatenate([reel, source]), np.array([0, 60, 660], dtype=np.int64))
al, s1, s8 = three_legs("reel_", reel_lib, np.tile(np.array([[0, 1]]), (4096, 1)), frames="60 x 600")
print(json.dumps(dict(leg="reel_summary", k8_over_align=s8["ms_median"] / al["ms_median"], bound_11_over_2=5.5)), flush=True)
reel_lib.free()
