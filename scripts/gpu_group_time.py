"""Times of the grouping on one MI355X, beside what it follows and what it saves: HIP events on the library
stream around the call, 3 warm-up runs, then the median of --reps runs with the min..max range, all in one process.
  python scripts/gpu_group_time.py [--reps 15] [--videos 50000] [--hashes 1000000] > group_time.jsonl
Legs:
  match_videos     the video search of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered on the
                   device): the records, and the time the grouping is an addition to
  group_records    hvd_dev_group_edges (HVD_EDGES_VMATCH, threshold 50, policy min, score = kept frames) over those records,
                   resident in HBM; checked once against search.similar_video_pairs + a host union-find
  allpairs         hvd_dev_allpairs_hamming256_mfma over --hashes clustered hashes (clusters of 100), the pairs left in HBM
  group_pairs      hvd_dev_group_edges over that resident pair list, behind the pass's own device-side count
  d2h_pairs        hvd_memcpy_d2h of the same pair list into pinned host memory (host clock around the synchronous copy): what
                   a caller pays today before it can group anything -- the figure to read first is group_over_d2h
Prints one JSON line per leg."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L, pipeline, search, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=50000)
ap.add_argument("--hashes", type=int, default=1_000_000)
args = ap.parse_args()
lib = L.init(0)
WARMUP = 3


def timed(fn):
    L.check(lib.hvd_timer_start())
    fn()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    return float(ms.value)


def host_timed(fn):
    L.check(lib.hvd_dev_sync())
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def leg(name, fn, clock=timed, **extra):
    for _ in range(WARMUP):
        fn()
    ms = [clock(fn) for _ in range(args.reps)]
    rec = dict(leg=name, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=args.reps, warmup=WARMUP, **extra)
    print(json.dumps(rec), flush=True)
    return rec


def host_components(pairs, V):
    parent = np.arange(V)
    for u, v in pairs:
        while parent[u] != u:
            u = parent[u]
        while parent[v] != v:
            v = parent[v]
        if u != v:
            parent[max(u, v)] = min(u, v)
    for v in range(V):
        parent[v] = parent[parent[v]]
    return parent


class Grouping:
    """The buffers of one hvd_dev_group_edges call over V nodes and up to n_records resident records."""

    def __init__(self, V, n_records):
        sb = C.c_size_t(0)
        L.check(lib.hvd_group_scratch_bytes(V, C.byref(sb)))
        self.V, self.cap = V, max(1, min(V // 2, n_records))
        self.bufs = [L.DeviceBuffer(sb.value), L.DeviceBuffer(4 * V), L.DeviceBuffer(16 * self.cap), L.DeviceBuffer(8)]

    def call(self, d_records, n_records, d_count, kind=L.EDGES_ALL, d_lengths=None, T=0, is_min=0, d_score=None):
        d_scr, d_label, d_groups, d_cnt = self.bufs
        L.check(lib.hvd_dev_group_edges(d_records, n_records, d_count, kind, d_lengths, T, is_min, self.V, d_score, d_scr.ptr,
                                        d_label.ptr, d_groups.ptr, self.cap, d_cnt.ptr))

    def read(self):
        n = int(self.bufs[3].to_array(np.uint64, 1)[0])
        return self.bufs[1].to_array(np.int32, self.V), self.bufs[2].to_array(L.GROUP_DTYPE, n)

    def free(self):
        for b in self.bufs:
            b.free()


# ---- leg 1: the config-5 library's records ----
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
lengths = library.lengths()
d_recs = L.DeviceBuffer.from_array(recs) if len(recs) else L.DeviceBuffer(16)
d_len = L.DeviceBuffer.from_array(lengths.astype(np.int64))
d_score = L.DeviceBuffer.from_array(lengths.astype(np.uint32))
g1 = Grouping(V, len(recs))
run1 = lambda: g1.call(d_recs.ptr, len(recs), None, L.EDGES_VMATCH, d_len.ptr, 50, 1, d_score.ptr)  # noqa: E731
run1()
labels, groups = g1.read()
assert np.array_equal(labels, host_components(search.similar_video_pairs(recs, lengths, 50.0, "min").tolist(), V))
grouped = leg("group_records", run1, records=len(recs), groups=len(groups), largest_group=int(groups["size"].max(initial=0)))
print(json.dumps(dict(leg="summary_records", group_over_search=grouped["ms_median"] / found["ms_median"])), flush=True)
for b in (d_recs, d_len, d_score):
    b.free()
g1.free()
library.free()

# ---- leg 2: the frame-level chain on clustered hashes ----
N = args.hashes
db, members = synth.hash_db_clustered(N, N // 1000, 100)
d_db = L.DeviceBuffer.from_array(db)
sz = C.c_size_t(0)
L.check(lib.hvd_fp4_image_bytes(N, C.byref(sz)))
d_img = L.DeviceBuffer(sz.value)
L.check(lib.hvd_dev_expand_fp4(d_db.ptr, N, d_img.ptr))
cap = 8 * N
d_pairs, d_cnt = L.DeviceBuffer(16 * cap), L.DeviceBuffer(8)


def allpairs():
    d_cnt.zero()
    L.check(lib.hvd_dev_allpairs_hamming256_mfma(d_db.ptr, d_img.ptr, N, None, 31, 0, 1, d_pairs.ptr, cap, d_cnt.ptr,
                                                 search.DEFAULT_VARIANT))


allpairs()
n_pairs = int(d_cnt.to_array(np.uint64, 1)[0])
assert n_pairs <= cap
passed = leg("allpairs", allpairs, hashes=N, pairs=n_pairs, pair_bytes=16 * n_pairs)
g2 = Grouping(N, cap)
run2 = lambda: g2.call(d_pairs.ptr, cap, d_cnt.ptr)  # noqa: E731
run2()
labels, groups = g2.read()
assert all(len(set(labels[c].tolist())) == 1 for c in members)
grouped = leg("group_pairs", run2, pairs=n_pairs, groups=len(groups), result_bytes=4 * N + 16 * len(groups))
h_pairs = C.c_void_p()
L.check(lib.hvd_host_malloc(C.byref(h_pairs), 16 * max(n_pairs, 1)))
copied = leg("d2h_pairs", lambda: L.check(lib.hvd_memcpy_d2h(h_pairs, d_pairs.ptr, 16 * n_pairs)), clock=host_timed,
             pair_bytes=16 * n_pairs)
L.check(lib.hvd_host_free(h_pairs))
print(json.dumps(dict(leg="summary_pairs", group_over_d2h=grouped["ms_median"] / copied["ms_median"],
                      group_over_allpairs=grouped["ms_median"] / passed["ms_median"])), flush=True)
g2.free()
for b in (d_db, d_img, d_pairs, d_cnt):
    b.free()
