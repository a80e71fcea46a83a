"""Times of the cover next to the plain alignment on one MI355X: HIP events on the library stream around the call,
3 warm-up runs, then the median of --reps runs with the min..max range. Everything sits in HBM.
  python scripts/gpu_cover_time.py [--reps 15] [--videos 50000] > cover_time.jsonl
Legs, all on the search records of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the device;
index positions, slack 1, min_aligned 4):
  align          hvd_dev_vpdq_align_videos: the two passes alone
  cover          hvd_dev_vpdq_cover_videos on the same records: the clear, the same two passes with the OR into the bitmap, the
                 count over the library's frames
  cover_floor_1  the same call at min_aligned 1: the records of this library are chance hits of a frame or two, none reaches
                 4 aligned frames, so only here does every pair with an aligned frame OR its words and count its sources
  library_cover  DeviceLibrary.cover, as a caller reaches it: the size query, four buffers, the entry, both read-backs
Prints one JSON line per leg and a summary with the ratios to `align`."""
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


V, F = args.videos, 64
n = V * F
d_frames = L.DeviceBuffer(n * 4096)
L.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, 0, V, F, 5, None))
d_h, d_q = pipeline.hash_frames_on_device(d_frames.ptr, n, 64, 64, 1)
library = pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, n, np.arange(V + 1, dtype=np.int64) * F)
for b in (d_frames, d_h, d_q):
    b.free()
recs = library.match_videos()
pairs = np.ascontiguousarray(np.stack([recs["a"], recs["b"]], axis=1), dtype=np.uint32)
M = len(pairs)
bins = 2 * int(library.lengths().max()) - 1 + 2
sb_al, sb_cov = C.c_size_t(0), C.c_size_t(0)
L.check(lib.hvd_align_scratch_bytes(bins, C.byref(sb_al)))
L.check(lib.hvd_cover_scratch_bytes(library.n_frames, bins, C.byref(sb_cov)))
d_pairs = L.DeviceBuffer.from_array(pairs)
d_out, d_out2 = L.DeviceBuffer(48 * max(M, 1)), L.DeviceBuffer(48 * max(M, 1))
d_cover = L.DeviceBuffer(16 * library.n_videos)
d_scr_al = L.DeviceBuffer(sb_al.value) if sb_al.value else None
d_scr_cov = L.DeviceBuffer(sb_cov.value)


def align():
    L.check(lib.hvd_dev_vpdq_align_videos(library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, None, library.d_hashes.ptr,
                                          library.d_offsets.ptr, library.n_videos, None, d_pairs.ptr, M, 31, 1,
                                          d_scr_al.ptr if d_scr_al else None, sb_al.value, d_out.ptr))


def cover(min_aligned=4):
    L.check(lib.hvd_dev_vpdq_cover_videos(library.d_hashes.ptr, library.d_offsets.ptr, library.n_videos, library.n_frames, None,
                                          d_pairs.ptr, M, 31, 1, min_aligned, d_scr_cov.ptr, sb_cov.value, d_out2.ptr, d_cover.ptr))


align()
cover(1)
cov1 = d_cover.to_array(L.VCOVER_DTYPE, library.n_videos)
cover()
al, al2 = d_out.to_array(L.VALIGN_DTYPE, M), d_out2.to_array(L.VALIGN_DTYPE, M)
cov = d_cover.to_array(L.VCOVER_DTYPE, library.n_videos)
assert np.array_equal(al, al2)
shape = dict(videos=V, kept_frames=library.n_frames, records=M, bitmap_bytes=sb_cov.value - sb_al.value,
             videos_with_a_source=int((cov["sources"] > 0).sum()), videos_beyond_one_partner=int((cov["covered"] > cov["best_single"]).sum()))
a = leg("align", align, **shape)
c = leg("cover", cover)
c1 = leg("cover_floor_1", lambda: cover(1), videos_with_a_source=int((cov1["sources"] > 0).sum()), sources=int(cov1["sources"].sum()),
         covered_frames=int(cov1["covered"].sum()))
w = leg("library_cover", lambda: library.cover(recs))
print(json.dumps(dict(leg="summary", align_ms=a["ms_median"], cover_ms=c["ms_median"], library_cover_ms=w["ms_median"],
                      cover_over_align=c["ms_median"] / a["ms_median"], cover_floor_1_over_align=c1["ms_median"] / a["ms_median"],
                      library_cover_over_align=w["ms_median"] / a["ms_median"])),
      flush=True)
library.free()
