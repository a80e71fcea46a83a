"""Times of the time alignment on one MI355X: HIP events on the library stream around the call, 3 warm-up runs,
then the median of --reps runs with the min..max range. Everything sits in HBM.
  python scripts/gpu_align_time.py [--reps 15] [--videos 50000] [--long 7200] > align_time.jsonl
Legs:
  match_videos   the video search of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
                 device): the candidates of the alignment, and the time it is an addition to
  align          hvd_dev_vpdq_align_videos of every record of that search (index positions, slack 1); comparisons per second
                 over 2 * sum(na * nb), and that rate as a fraction of ...
  popcount       ... the integer all-pairs kernel (variant 0) on the first 262 144 kept hashes of the same library
  align_long     one pair of two --long-frame videos (a copy with up to 24 flipped bits per frame): one pair is one workgroup
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
ap.add_argument("--long", type=int, default=7200)
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
    rec = dict(leg=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=args.reps, warmup=WARMUP)
    for k, v in extra.items():
        rec[k] = v(rec["ms_median"]) if callable(v) else v
    print(json.dumps(rec), flush=True)
    return rec


def align_call(library, pairs, slack=1):
    """Buffers of one hvd_dev_vpdq_align_videos call over `library` against itself, and the call."""
    M = len(pairs)
    bins = 2 * int(library.lengths().max()) - 1 + 2 * slack
    sb = C.c_size_t(0)
    L.check(lib.hvd_align_scratch_bytes(min(bins, L.ALIGN_MAX_BINS), C.byref(sb)))
    d_pairs = L.DeviceBuffer.from_array(np.ascontiguousarray(pairs, dtype=np.uint32))
    d_out = L.DeviceBuffer(L.VALIGN_DTYPE.itemsize * max(M, 1))
    d_scr = L.DeviceBuffer(sb.value) if sb.value else None

    def call():
        L.check(lib.hvd_dev_vpdq_align_videos(library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, None,
                                              library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, None, d_pairs.ptr,
                                              M, 31, slack, d_scr.ptr if d_scr else None, sb.value, d_out.ptr))

    return call, d_out, (d_pairs, d_out, d_scr)


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

lengths = library.lengths()
pairs = np.stack([recs["a"], recs["b"]], axis=1)
cmp_align = 2.0 * float((lengths[recs["a"]] * lengths[recs["b"]]).sum())
call, d_out, bufs = align_call(library, pairs)
call()
al = d_out.to_array(L.VALIGN_DTYPE, len(pairs))
assert np.array_equal(al["q_hits"], recs["q_hits"]) and np.array_equal(al["t_hits"], recs["t_hits"])
align = leg("align", call, pairs=len(pairs), comparisons=cmp_align, cmp_per_s=lambda ms: cmp_align / (ms * 1e-3),
            aligned_ge_half=int((2 * np.maximum(al["q_aligned"], al["t_aligned"]) >= 64).sum()))
for b in bufs:
    if b is not None:
        b.free()

npop = min(library.n_frames, 1 << 18)
cap = 1 << 22
d_fp, d_cnt = L.DeviceBuffer(16 * cap), L.DeviceBuffer(8)


def popcount():
    d_cnt.zero()
    L.check(lib.hvd_dev_allpairs_hamming256(library.d_hashes.ptr, npop, library.d_video.ptr, 31, 0, 1, d_fp.ptr, cap, d_cnt.ptr, 0))


cmp_pop = npop * (npop - 1) / 2.0
pop = leg("popcount", popcount, hashes=npop, comparisons=cmp_pop, cmp_per_s=lambda ms: cmp_pop / (ms * 1e-3))
print(json.dumps(dict(leg="summary", align_ms=align["ms_median"], match_videos_ms=search["ms_median"],
                      align_over_search=align["ms_median"] / search["ms_median"],
                      align_rate_over_popcount_rate=align["cmp_per_s"] / pop["cmp_per_s"])), flush=True)
library.free()

# ---- one long pair: one workgroup ----
N = args.long
base = synth.hash_db(N, seed=9, plant_fraction=0.0)[0]
rng = np.random.default_rng(9)
copy = synth.flip_bits(base, rng.integers(0, 25, N), rng)
long_lib = pipeline.DeviceLibrary.from_host(np.concatenate([base, copy]), np.array([0, N, 2 * N], dtype=np.int64))
call, d_out, bufs = align_call(long_lib, np.array([[0, 1]]))
call()
r = d_out.to_array(L.VALIGN_DTYPE, 1)[0]
assert (int(r["offset"]), int(r["q_aligned"]), int(r["t_aligned"])) == (0, N, N), r
cmp_long = 2.0 * N * N
leg("align_long", call, frames=N, comparisons=cmp_long, cmp_per_s=lambda ms: cmp_long / (ms * 1e-3))
