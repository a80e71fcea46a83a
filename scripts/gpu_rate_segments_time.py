"""Times of the rate-aware multi-segment alignment on one MI355X, beside the two calls it joins: HIP events on the
library stream around the call, 3 warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_rate_segments_time.py [--reps 15] [--videos 50000] > rate_segments_time.jsonl
Legs:
  match_videos        the video search of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
                      device): the candidates
  segments_k8         hvd_dev_vpdq_align_segments of every record of that search (index positions, slack 1, K = 8,
                      min_band_votes = 4)
  rates_r8            hvd_dev_vpdq_align_rates of the same records under the eight default rates
  rate_segments_r8k8  hvd_dev_vpdq_align_rate_segments of the same records (R = 8, K = 8, min_band_votes = 4). The candidates
                      are full copies that end in one round: the call should cost about what rates_r8 costs
  reel_*              4 096 copies of one pair through the same three: a 150-frame reel of four pieces at 3/2, 2/1, 1/1 and 5/4
                      against its 600-frame source. Four rounds; the bound-skip decides how many of the 4 x 9 passes are made
Every ratio is new / rates_r8 and new / segments_k8 of the same process. Prints one JSON line per leg."""
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
RATES = search.rate_array(search.DEFAULT_RATES)
K, FLOOR = 8, 4


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


def three_legs(prefix, library, pairs, slack=1, **extra):
    """The three calls over `library` against itself on one set of buffers; their records are checked against each other
    before anything is timed. -> the three leg records."""
    M = len(pairs)
    span = int(library.lengths().max()) - 1
    bins = min(max((n + d) * span + 1 + 2 * slack * max(n, d) for n, d in search.DEFAULT_RATES), L.ALIGN_MAX_BINS)
    sb = C.c_size_t(0)
    L.check(lib.hvd_rate_segments_scratch_bytes(bins, C.byref(sb)))  # (serves all three: the most runs of bit words, the most bins)
    d_pairs = L.DeviceBuffer.from_array(np.ascontiguousarray(pairs, dtype=np.uint32))
    d_out = L.DeviceBuffer(L.VRSEGMENTS_DTYPE.itemsize * max(M, 1))
    d_scr = L.DeviceBuffer(sb.value) if sb.value else None
    h, o, V, scr = library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, d_scr.ptr if d_scr else None

    def segments():
        L.check(lib.hvd_dev_vpdq_align_segments(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, K, FLOOR, scr, sb.value,
                                                d_out.ptr))

    def rates():
        L.check(lib.hvd_dev_vpdq_align_rates(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, RATES.ctypes.data, len(RATES),
                                             scr, sb.value, d_out.ptr))

    def both(k=K, floor=FLOOR):
        L.check(lib.hvd_dev_vpdq_align_rate_segments(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, RATES.ctypes.data,
                                                     len(RATES), k, floor, scr, sb.value, d_out.ptr))

    def read(fn, dtype):
        fn()
        return d_out.to_array(dtype, M)

    sg, rt, new = read(segments, L.VSEGMENTS_DTYPE), read(rates, L.VRATE_DTYPE), read(both, L.VRSEGMENTS_DTYPE)
    one = read(lambda: both(1, 1), L.VRSEGMENTS_DTYPE)
    for f in L.VRATE_DTYPE.names[4:]:  # one segment, no floor: the rate record
        assert np.array_equal(one["seg"][:, 0][f], rt[f]), f
    assert np.array_equal(new["q_hits"], rt["q_hits"]) and np.array_equal(new["q_hits"], sg["q_hits"])
    first = new["n_segments"] > 0
    assert np.array_equal(new["seg"][:, 0]["band_votes"][first], rt["band_votes"][first])
    out = [leg(prefix + "segments_k8", segments, pairs=M, segments_found=int(sg["n_segments"].sum()),
               covered_frames=int(sg["q_covered"].sum()), **extra),
           leg(prefix + "rates_r8", rates, pairs=M, matrix_passes_per_pair=9, aligned_frames=int(rt["q_aligned"].sum())),
           leg(prefix + "rate_segments_r8k8", both, pairs=M, largest_bins=bins, segments_found=int(new["n_segments"].sum()),
               pairs_by_segments=np.bincount(new["n_segments"], minlength=K + 1).tolist(), covered_frames=int(new["q_covered"].sum()),
               matrix_passes_per_pair_at_most=K * (len(RATES) + 1))]
    for b in (d_pairs, d_out, d_scr):
        if b is not None:
            b.free()
    return out


def summary(name, sg, rt, new, **extra):
    print(json.dumps(dict(leg=name, new_over_rates=new["ms_median"] / rt["ms_median"], new_over_segments=new["ms_median"] / sg["ms_median"],
                          **extra)), flush=True)


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
sg, rt, new = three_legs("", library, np.stack([recs["a"], recs["b"]], axis=1))
summary("summary", sg, rt, new, new_over_search=new["ms_median"] / found["ms_median"],
        expectation="full copies end in one round: new / rates_r8 about 1")
library.free()

# ---- a reel whose pieces were sped up: four pieces at four rates of a 600-frame source ----
rng = np.random.default_rng(91)
source = synth.hash_db(600, seed=91, plant_fraction=0.0)[0]
idx = lambda m, num, den, c: np.floor(np.arange(m) * num / den + c + 0.5).astype(np.int64)  # noqa: E731
cut = np.concatenate([idx(40, 3, 2, 300.3), idx(30, 2, 1, 50.6), idx(20, 1, 1, 500.0), idx(60, 5, 4, 400.2)])
reel = synth.flip_bits(source[cut], rng.integers(0, 21, len(cut)), rng)
reel_lib = pipeline.DeviceLibrary.from_host(np.concatenate([reel, source]), np.array([0, 150, 750], dtype=np.int64))
sg, rt, new = three_legs("reel_", reel_lib, np.tile(np.array([[0, 1]]), (4096, 1)), frames="150 x 600, pieces at 3/2, 2/1, 1/1, 5/4")
summary("reel_summary", sg, rt, new, passes_unpruned=4 * 9, passes_rates=9)
reel_lib.free()
