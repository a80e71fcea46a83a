"""Times of the time alignment with negative rates on one MI355X, beside the calls it generalises: HIP events on the
library stream around the call, 3 warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_signed_time.py [--reps 15] [--videos 50000] > signed_time.jsonl
Legs, on the records of the config-5 library's video search (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
device) and on 4 096 copies of one planted reversed-reel pair (a 110-frame reel -- 40 frames forward, 40 reversed, 30 reversed
at 2x -- against its 600-frame source):
  rate_segments_fwd2  hvd_dev_vpdq_align_rate_segments under ((1, 1), (2, 1)), K = 8, min_band_votes = 4
  signed_fwd2         hvd_dev_vpdq_align_signed under the same all-positive list: the price of the generality. The passes are
                      the same from the code, so the expectation is 1.0x; the records are checked to be the same words
  rate_segments_fwd2_again   the first leg once more: the spread two runs of one kernel show in one process
  segments_k8         hvd_dev_vpdq_align_segments at the same K and floor
  signed_reversed     hvd_dev_vpdq_align_signed under REVERSED_RATES ((1, 1), (-1, 1)): R + 1 = 3 passes over a pair that ends in
                      one round where segments_k8 makes 2, so the expectation is 1.5x of its passes
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
FWD2 = search.rate_array(((1, 1), (2, 1)))
REV = search.rate_array(search.REVERSED_RATES)
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


def legs(prefix, library, pairs, slack=1, **extra):
    """The calls over `library` against itself on one set of buffers; the records of the two forward legs are checked to be
    the same words before anything is timed."""
    M = len(pairs)
    span = int(library.lengths().max()) - 1
    bins = min(3 * span + 1 + 4 * slack, L.ALIGN_MAX_BINS)  # (2, 1): the widest listed rate
    sb = C.c_size_t(0)
    L.check(lib.hvd_signed_scratch_bytes(bins, C.byref(sb)))  # (serves every leg: two pairs of runs of bit words, the most bins)
    d_pairs = L.DeviceBuffer.from_array(np.ascontiguousarray(pairs, dtype=np.uint32))
    d_out = L.DeviceBuffer(L.VSSEGMENTS_DTYPE.itemsize * max(M, 1))
    d_scr = L.DeviceBuffer(sb.value) if sb.value else None
    h, o, V, scr = library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, d_scr.ptr if d_scr else None

    def segments():
        L.check(lib.hvd_dev_vpdq_align_segments(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, K, FLOOR, scr, sb.value,
                                                d_out.ptr))

    def rated(entry, rates):
        def call():
            L.check(getattr(lib, entry)(h, o, V, None, h, o, V, None, d_pairs.ptr, M, 31, slack, rates.ctypes.data, len(rates), K,
                                        FLOOR, scr, sb.value, d_out.ptr))
        return call

    def read(fn, dtype):
        fn()
        return d_out.to_array(dtype, M)

    fwd_call, sgn_call = rated("hvd_dev_vpdq_align_rate_segments", FWD2), rated("hvd_dev_vpdq_align_signed", FWD2)
    rev_call = rated("hvd_dev_vpdq_align_signed", REV)
    fwd, sgn = read(fwd_call, L.VRSEGMENTS_DTYPE), read(sgn_call, L.VSSEGMENTS_DTYPE)
    assert np.array_equal(fwd.view(np.uint32), sgn.view(np.uint32))
    sg, rev = read(segments, L.VSEGMENTS_DTYPE), read(rev_call, L.VSSEGMENTS_DTYPE)
    assert np.array_equal(rev["q_hits"], sg["q_hits"])
    out = dict(
        fwd=leg(prefix + "rate_segments_fwd2", fwd_call, pairs=M, largest_bins=bins, segments_found=int(fwd["n_segments"].sum()), **extra),
        sgn=leg(prefix + "signed_fwd2", sgn_call, pairs=M, segments_found=int(sgn["n_segments"].sum())),
        again=leg(prefix + "rate_segments_fwd2_again", fwd_call, pairs=M),
        sg=leg(prefix + "segments_k8", segments, pairs=M, segments_found=int(sg["n_segments"].sum()), covered_frames=int(sg["q_covered"].sum())),
        rev=leg(prefix + "signed_reversed", rev_call, pairs=M, segments_found=int(rev["n_segments"].sum()),
                covered_frames=int(rev["q_covered"].sum()), reversed_segments=int((rev["seg"]["rate_num"] < 0).sum())))
    print(json.dumps(dict(leg=prefix + "summary", signed_over_rate_segments=out["sgn"]["ms_median"] / out["fwd"]["ms_median"],
                          again_over_first=out["again"]["ms_median"] / out["fwd"]["ms_median"],
                          reversed_over_segments=out["rev"]["ms_median"] / out["sg"]["ms_median"],
                          expectation="signed_over_rate_segments 1.0; reversed_over_segments 1.5 where a pair ends in one round")),
          flush=True)
    for b in (d_pairs, d_out, d_scr):
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

# ---- a reel with reversed pieces: 40 frames forward, 40 reversed, 30 reversed at 2x, of a 600-frame source ----
rng = np.random.default_rng(70)
source = synth.hash_db(600, seed=70, plant_fraction=0.0)[0]
back = lambda m, num, c: np.floor(c - np.arange(m) * num + 0.5).astype(np.int64)  # noqa: E731
cut = np.concatenate([np.arange(50, 90), np.arange(400, 440)[::-1], back(30, 2, 299.6)])
reel = synth.flip_bits(source[cut], rng.integers(0, 21, len(cut)), rng)
reel_lib = pipeline.DeviceLibrary.from_host(np.concatenate([reel, source]), np.array([0, 110, 710], dtype=np.int64))
legs("reel_", reel_lib, np.tile(np.array([[0, 1]]), (4096, 1)), frames="110 x 600: forward, reversed, reversed at 2x")
reel_lib.free()
