"""Times of the time alignment of looped clips on one MI355X, beside the signed entry it is derived from: HIP events
on the library stream around the call, 3 warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_loops_time.py [--reps 15] [--videos 50000] > loops_time.jsonl
Legs, on the records of the config-5 library's video search (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
device; at a floor of 4 none of them makes a round, so these legs compare pass 1 and a pair's fixed work), on 4 096 copies of a
plain 60-frame excerpt against its 600-frame source (every pair ends after exactly ONE round in both entries) and on 4 096
copies of a looped pair (300 frames = five repetitions of a 60-frame moment, against the same source), all under REVERSED_RATES
((1, 1), (-1, 1)) with a floor of 4 hits:
  signed          hvd_dev_vpdq_align_signed, K = 8
  loops           hvd_dev_vpdq_align_loops, max_rounds = 64, one orientation: on pairs that make no round or end in one the passes
                  are the signed entry's, so the expectation is 1.0x, plus the one count of the seen words on the excerpt; on the
                  looped pair it makes five rounds where the signed entry makes two (the second finds nothing), so it costs
                  its rounds
  signed_again    the first leg once more: the spread two runs of one kernel show in one process
  loops_both      hvd_dev_vpdq_align_loops on (a, b) and (b, a), twice the pairs, as find_looped_excerpts calls it: about 2x
Every ratio is taken inside one process. Prints one JSON line per leg."""
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
REV = search.rate_array(search.REVERSED_RATES)
K, ROUNDS, FLOOR = 8, L.ALIGN_MAX_ROUNDS, 4


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


def legs(prefix, library, pairs, slack=1, **extra):
    """The calls over `library` against itself on one set of buffers; seg[0] and the hit counts of the two entries are checked
    to be the same words before anything is timed."""
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32)
    both = np.ascontiguousarray(np.concatenate([pairs, pairs[:, ::-1]]))
    M = len(pairs)
    span = int(library.lengths().max()) - 1
    bins = min(2 * span + 1 + 2 * slack, L.ALIGN_MAX_BINS)
    sb = C.c_size_t(0)
    L.check(lib.hvd_loops_scratch_bytes(bins, C.byref(sb)))  # (serves every leg: three pairs of runs of bit words)
    d_pairs, d_both = L.DeviceBuffer.from_array(pairs), L.DeviceBuffer.from_array(both)
    d_out = L.DeviceBuffer(L.VLOOPS_DTYPE.itemsize * max(2 * M, 1))
    d_scr = L.DeviceBuffer(sb.value) if sb.value else None
    h, o, V, scr = library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, d_scr.ptr if d_scr else None

    def call(entry, d_list, n, limit):
        def run():
            L.check(getattr(lib, entry)(h, o, V, None, h, o, V, None, d_list.ptr, n, 31, slack, REV.ctypes.data, len(REV), limit, FLOOR,
                                        scr, sb.value, d_out.ptr))
        return run

    def read(fn, dtype, n):
        fn()
        return d_out.to_array(dtype, n)

    sgn_call = call("hvd_dev_vpdq_align_signed", d_pairs, M, K)
    one_call = call("hvd_dev_vpdq_align_loops", d_pairs, M, ROUNDS)
    both_call = call("hvd_dev_vpdq_align_loops", d_both, 2 * M, ROUNDS)
    sgn, one = read(sgn_call, L.VSSEGMENTS_DTYPE, M), read(one_call, L.VLOOPS_DTYPE, M)
    assert np.array_equal(sgn["q_hits"], one["q_hits"]) and np.array_equal(sgn["seg"][:, 0], one["seg"][:, 0])
    two = read(both_call, L.VLOOPS_DTYPE, 2 * M)
    assert np.array_equal(two[:M], one)
    out = dict(
        sgn=leg(prefix + "signed", sgn_call, pairs=M, largest_bins=bins, segments_found=int(sgn["n_segments"].sum()),
                covered_frames=int(sgn["q_covered"].sum()), **extra),
        one=leg(prefix + "loops", one_call, pairs=M, rounds_made=int(one["rounds"].sum()), covered_frames=int(one["q_covered"].sum()),
                pairs_past_one_round=int((one["rounds"] > 1).sum())),
        again=leg(prefix + "signed_again", sgn_call, pairs=M),
        both=leg(prefix + "loops_both", both_call, pairs=2 * M, rounds_made=int(two["rounds"].sum())))
    print(json.dumps(dict(leg=prefix + "summary", loops_over_signed=out["one"]["ms_median"] / out["sgn"]["ms_median"],
                          again_over_first=out["again"]["ms_median"] / out["sgn"]["ms_median"],
                          both_over_signed=out["both"]["ms_median"] / out["sgn"]["ms_median"],
                          both_over_loops=out["both"]["ms_median"] / out["one"]["ms_median"],
                          expectation="loops_over_signed 1.0 where pairs make no round or end in one; both_over_loops 2.0 where the "
                                      "two orientations cost alike; the looped pair costs its five rounds")), flush=True)
    for b in (d_pairs, d_both, d_out, d_scr):
        if b is not None:
            b.free()


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
legs("", library, np.stack([recs["a"], recs["b"]], axis=1), videos=V, records=len(recs))
library.free()

# ---- a plain excerpt: 60 frames of a 600-frame source, one round in either entry ----
rng = np.random.default_rng(71)
source = synth.hash_db(600, seed=71, plant_fraction=0.0)[0]
clip = synth.flip_bits(source[200:260], rng.integers(0, 21, 60), rng)
clip_lib = pipeline.DeviceLibrary.from_host(np.concatenate([clip, source]), np.array([0, 60, 660], dtype=np.int64))
legs("clip_", clip_lib, np.tile(np.array([[0, 1]]), (4096, 1)), frames="60 x 600: a plain excerpt, one round")
clip_lib.free()

# ---- a five-fold loop: 300 frames = 5 x 60 of the same source ----
cut = np.tile(np.arange(100, 160), 5)
loop5 = synth.flip_bits(source[cut], rng.integers(0, 21, len(cut)), rng)
loop_lib = pipeline.DeviceLibrary.from_host(np.concatenate([loop5, source]), np.array([0, 300, 900], dtype=np.int64))
legs("loop5_", loop_lib, np.tile(np.array([[0, 1]]), (4096, 1)), frames="300 x 600: a 60-frame moment five times")
loop_lib.free()
