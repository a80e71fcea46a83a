"""Times of the keeper-first grouping on one MI355X beside the components call it stands next to: HIP events on
the library stream around each call plus the host clock around call + synchronise (hvd_dev_keeper_groups synchronises between
its batches of rounds, so its host time is part of what a caller pays), 3 warm-up runs, then the median of --reps runs with the
min..max range, both entries over the same resident records in one process.
  python scripts/gpu_keeper_time.py [--reps 15] [--videos 50000] [--hashes 1000000] > keeper_time.jsonl
Legs:
  match_videos          the video search of the config-5 library (--videos x 64 synthetic 64x64 frames, hashed and filtered
                        on the device): the records, and the time either grouping is an addition to
  group_records         hvd_dev_group_edges (HVD_EDGES_VMATCH, threshold 50, policy min, score = kept frames) over them
  keeper_records        hvd_dev_keeper_groups over the same records and operands; its result is checked once: every member
                        has an edge to its keeper, no two keepers share an edge
  group_pairs           hvd_dev_group_edges over the resident pair list of --hashes clustered hashes (clusters of 100)
  keeper_pairs          hvd_dev_keeper_groups over that list, with random scores (as resolution or file size would be) and
                        with none (index priority inside every cluster)
Prints one JSON line per leg; keeper_over_group is the ratio of the medians of the event times."""
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


def both_clocks(fn):
    """-> (event ms, host ms): HIP events around the enqueued work; the host clock from a quiet stream to a quiet stream."""
    L.check(lib.hvd_dev_sync())
    t0 = time.perf_counter()
    L.check(lib.hvd_timer_start())
    fn()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    L.check(lib.hvd_dev_sync())
    return float(ms.value), (time.perf_counter() - t0) * 1e3


def leg(name, fn, **extra):
    for _ in range(WARMUP):
        fn()
    ev, host = zip(*[both_clocks(fn) for _ in range(args.reps)])
    rec = dict(leg=name, ms_median=statistics.median(ev), ms_min=min(ev), ms_max=max(ev), host_ms_median=statistics.median(host),
               host_ms_min=min(host), host_ms_max=max(host), reps=args.reps, warmup=WARMUP, **extra)
    print(json.dumps(rec), flush=True)
    return rec


class Grouping:
    """The buffers of one grouping call of either kind over V nodes and up to n_records resident records."""

    def __init__(self, V, n_records, keeper_first):
        sb = C.c_size_t(0)
        L.check((lib.hvd_keeper_scratch_bytes if keeper_first else lib.hvd_group_scratch_bytes)(V, C.byref(sb)))
        self.V, self.cap, self.keeper_first, self.rounds = V, max(1, min(V // 2, n_records)), keeper_first, C.c_int64(0)
        self.bufs = [L.DeviceBuffer(sb.value), L.DeviceBuffer(4 * V), L.DeviceBuffer(16 * self.cap), L.DeviceBuffer(8)]

    def call(self, d_records, n_records, d_count, kind=L.EDGES_ALL, d_lengths=None, T=0, is_min=0, d_score=None):
        d_scr, d_node, d_groups, d_cnt = self.bufs
        head = (d_records, n_records, d_count, kind, d_lengths, T, is_min, self.V, d_score, d_scr.ptr, d_node.ptr, d_groups.ptr,
                self.cap, d_cnt.ptr)
        if self.keeper_first:
            L.check(lib.hvd_dev_keeper_groups(*head, C.byref(self.rounds)))
        else:
            L.check(lib.hvd_dev_group_edges(*head))

    def read(self):
        n = int(self.bufs[3].to_array(np.uint64, 1)[0])
        return self.bufs[1].to_array(np.int32, self.V), self.bufs[2].to_array(L.GROUP_DTYPE, n)

    def free(self):
        for b in self.bufs:
            b.free()


def check_promises(keeper_of, uv):
    """(a) every member has an edge to its keeper; (b) no two keepers share an edge. uv: int64[E, 2], the edges."""
    keeper_of = keeper_of.astype(np.int64)
    is_keeper = keeper_of == np.arange(len(keeper_of))
    direct = np.zeros(len(keeper_of), dtype=bool)
    direct[uv[keeper_of[uv[:, 0]] == uv[:, 1], 0]] = True
    direct[uv[keeper_of[uv[:, 1]] == uv[:, 0], 1]] = True
    assert np.array_equal(direct, ~is_keeper) and not (is_keeper[uv[:, 0]] & is_keeper[uv[:, 1]]).any()


def compare(name, grouped, kept, rounds, **extra):
    print(json.dumps(dict(leg=name, keeper_over_group=kept["ms_median"] / grouped["ms_median"],
                          keeper_over_group_host=kept["host_ms_median"] / grouped["host_ms_median"], rounds=rounds, **extra)), flush=True)


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
operands = (d_recs.ptr, len(recs), None, L.EDGES_VMATCH, d_len.ptr, 50, 1, d_score.ptr)
g1, k1 = Grouping(V, len(recs), False), Grouping(V, len(recs), True)
k1.call(*operands)
keeper_of, groups = k1.read()
check_promises(keeper_of, search.similar_video_pairs(recs, lengths, 50.0, "min"))
grouped = leg("group_records", lambda: g1.call(*operands), records=len(recs))
kept = leg("keeper_records", lambda: k1.call(*operands), records=len(recs), groups=len(groups), rounds=k1.rounds.value,
           largest_group=int(groups["size"].max(initial=0)))
compare("summary_records", grouped, kept, k1.rounds.value, keeper_over_search=kept["ms_median"] / found["ms_median"])
for b in (d_recs, d_len, d_score):
    b.free()
g1.free()
k1.free()
library.free()

# ---- leg 2: the resident pair list of clustered hashes ----
N = args.hashes
db, members = synth.hash_db_clustered(N, N // 1000, 100)
d_db = L.DeviceBuffer.from_array(db)
sz = C.c_size_t(0)
L.check(lib.hvd_fp4_image_bytes(N, C.byref(sz)))
d_img = L.DeviceBuffer(sz.value)
L.check(lib.hvd_dev_expand_fp4(d_db.ptr, N, d_img.ptr))
cap = 8 * N
d_pairs, d_cnt = L.DeviceBuffer(16 * cap), L.DeviceBuffer(8)
d_cnt.zero()
L.check(lib.hvd_dev_allpairs_hamming256_mfma(d_db.ptr, d_img.ptr, N, None, 31, 0, 1, d_pairs.ptr, cap, d_cnt.ptr, search.DEFAULT_VARIANT))
n_pairs = int(d_cnt.to_array(np.uint64, 1)[0])
assert n_pairs <= cap
uv = d_pairs.to_array(L.PAIR_DTYPE, n_pairs)
uv = np.stack([uv["i"], uv["j"]], axis=1).astype(np.int64)
d_rand = L.DeviceBuffer.from_array(np.random.default_rng(14).integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32))
g2, k2 = Grouping(N, cap, False), Grouping(N, cap, True)
grouped = leg("group_pairs", lambda: g2.call(d_pairs.ptr, cap, d_cnt.ptr), hashes=N, pairs=n_pairs)
for name, d_sc in (("keeper_pairs_random_scores", d_rand.ptr), ("keeper_pairs_no_scores", None)):
    run = lambda: k2.call(d_pairs.ptr, cap, d_cnt.ptr, d_score=d_sc)  # noqa: E731
    run()
    keeper_of, groups = k2.read()
    check_promises(keeper_of, uv)
    kept = leg(name, run, pairs=n_pairs, groups=len(groups), rounds=k2.rounds.value)
    compare("summary_" + name, grouped, kept, k2.rounds.value)
g2.free()
k2.free()
for b in (d_db, d_img, d_pairs, d_cnt, d_rand):
    b.free()
