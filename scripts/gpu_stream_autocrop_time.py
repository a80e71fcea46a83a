"""Times of the fused rectangle down-sampler and of the autocrop streaming hasher on one MI355X. Device legs:
HIP events on the library stream around each call; streamed legs: host wall time. 3 warm-up runs, then the median of --reps
runs with min .. max, all legs interleaved in one process. One JSON line per leg.
  python scripts/gpu_stream_autocrop_time.py [--reps 15] [--videos 128] [--stream-frames 300]
1. hvd_dev_pdq_hash_frames_rects on --videos x 48 frames of 512x512 RGB24 in HBM (6 144 by default), 64-row bars and no
   bars, with the debug key pdq_fused_rect at 1 (k_down_rect) and at 0 (the four generic passes), next to
   hvd_dev_pdq_hash_frames on the unbarred frames with the wave-per-frame kernel (default) and with the workgroup-per-frame
   k_down512<3, 32> (pdq_down512_wave 0), the yardstick for a workgroup-per-frame form.
2. The same on the first --stream-frames frames (what finish() of a streamed video launches).
3. One VideoHasher per video, hash_frame(bytes), --stream-frames frames: plain, autocrop with 64-row bars, autocrop without
   bars, and both autocrop legs again with pdq_fused_rect 0; finish()'s own wall time is reported per leg."""
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
from hvd_amd import _lib as L, vpdq  # noqa: E402

READ_LOOP_TBS = (5.9, 6.15)  # profiles/r05_fetch_calibration.txt: the bare read loop on this class of box

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=128)
ap.add_argument("--stream-frames", type=int, default=300)
args = ap.parse_args()
lib = L.init(0)
H = W = 512
FPV = 48
V, N = args.videos, args.videos * FPV
SF = args.stream_frames
assert SF <= N
rng = np.random.default_rng(1)


def video(bars, frames=FPV):
    one = rng.integers(0, 9, (frames, H, W, 3), dtype=np.uint8)
    one[:, bars:H - bars] = rng.integers(40, 256, (frames, H - 2 * bars, W, 3), dtype=np.uint8)
    return one


def library(bars):
    """V videos in HBM: one 48-frame video made on the host, copied V times on the device."""
    one = video(bars)
    d_one = L.DeviceBuffer.from_array(one)
    d_all = L.DeviceBuffer(one.nbytes * V)
    for v in range(V):
        L.check(lib.hvd_memcpy_d2d(d_all.ptr + one.nbytes * v, d_one.ptr, one.nbytes))
    L.check(lib.hvd_dev_sync())
    d_one.free()
    return d_all


def timed(fn):
    L.check(lib.hvd_timer_start())
    fn()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    return float(ms.value)


d_bar, d_full = library(64), library(0)
d_off = L.DeviceBuffer.from_array(np.array([0, N], dtype=np.int64))  # one rectangle for all frames: what a hasher has
d_rc = {64: L.DeviceBuffer.from_array(np.array([64, 0, H - 128, W], np.int32)),
        0: L.DeviceBuffer.from_array(np.array([0, 0, H, W], np.int32))}
d_h, d_q = L.DeviceBuffer(32 * N), L.DeviceBuffer(4 * N)
sb = C.c_size_t(0)
L.check(lib.hvd_pdq_rects_scratch_bytes(N, H, W, 3, C.byref(sb)))
d_s = L.DeviceBuffer(sb.value)


def hash_rects(d_fr, bars, n, fused):
    L.check(lib.hvd_debug_set(b"pdq_fused_rect", fused))
    L.check(lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, n, H, W, 3, d_off.ptr, 1, d_rc[bars].ptr, d_s.ptr, d_h.ptr, d_q.ptr))
    L.check(lib.hvd_debug_set(b"pdq_fused_rect", 1))


def plain(n, wave):
    L.check(lib.hvd_debug_set(b"pdq_down512_wave", wave))
    L.check(lib.hvd_dev_pdq_hash_frames(d_full.ptr, n, H, W, 3, d_s.ptr, d_h.ptr, d_q.ptr))
    L.check(lib.hvd_debug_set(b"pdq_down512_wave", 1))


device_legs = {}
for n in (N, SF):
    device_legs.update({
        (n, "rects_fused_barred"): lambda n=n: hash_rects(d_bar, 64, n, 1),
        (n, "rects_generic_barred"): lambda n=n: hash_rects(d_bar, 64, n, 0),
        (n, "rects_fused_unbarred"): lambda n=n: hash_rects(d_full, 0, n, 1),
        (n, "rects_generic_unbarred"): lambda n=n: hash_rects(d_full, 0, n, 0),
        (n, "plain_unbarred"): lambda n=n: plain(n, 1),
        (n, "plain_unbarred_workgroup_form"): lambda n=n: plain(n, 0),
    })
times = {k: [] for k in device_legs}
for rep in range(3 + args.reps):
    for k, fn in device_legs.items():
        ms = timed(fn)
        if rep >= 3:
            times[k].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
for (n, leg), v in times.items():
    rec = {"leg": leg, "frames": n, "geometry": "512x512 rgb24", "what": "call time, HIP events on the library stream",
           "median_ms": round(med[(n, leg)], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}
    if leg.startswith("rects_fused"):
        rows = H - 128 if leg.endswith("_barred") else H
        nbytes = n * rows * W * 3  # the bytes of the rectangle's rows
        tbs = nbytes / (med[(n, leg)] * 1e-3) / 1e12
        rec.update(rect_bytes=nbytes, tb_per_s=round(tbs, 3), share_of_read_loop=[round(tbs / x, 3) for x in READ_LOOP_TBS],
                   generic_over_fused=round(med[(n, leg.replace("fused", "generic"))] / med[(n, leg)], 3),
                   fused_over_workgroup_form=round(med[(n, leg)] / med[(n, "plain_unbarred_workgroup_form")], 3))
    print(json.dumps(rec), flush=True)
for b in (d_bar, d_full, d_s, d_h, d_q, d_off, *d_rc.values()):
    b.free()

# ---- the reference call pattern: one hasher per video, hash_frame(bytes) ----
if SF > 0:
    vids = {64: [f.tobytes() for f in video(64, SF)], 0: [f.tobytes() for f in video(0, SF)]}

    def stream(bars, autocrop, fused):
        L.check(lib.hvd_debug_set(b"pdq_fused_rect", fused))
        t0 = time.perf_counter()
        hs = vpdq.VideoHasher(1, W, H, 0, autocrop=autocrop)
        for f in vids[bars]:
            hs.hash_frame(f)
        t1 = time.perf_counter()
        hs.finish()
        t2 = time.perf_counter()
        L.check(lib.hvd_debug_set(b"pdq_fused_rect", 1))
        if autocrop:
            assert hs.rect == (bars, 0, H - 2 * bars, W), hs.rect
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    stream_legs = {
        "plain": lambda: stream(64, None, 1),
        "autocrop_barred": lambda: stream(64, True, 1),
        "autocrop_unbarred": lambda: stream(0, True, 1),
        "autocrop_barred_generic": lambda: stream(64, True, 0),
        "autocrop_unbarred_generic": lambda: stream(0, True, 0),
    }
    runs = {k: [] for k in stream_legs}
    for rep in range(3 + args.reps):
        for k, fn in stream_legs.items():
            r = fn()
            if rep >= 3:
                runs[k].append(r)
    base = statistics.median(t for t, _ in runs["plain"])
    for k, rs in runs.items():
        tot, fin = [t for t, _ in rs], [f for _, f in rs]
        print(json.dumps({"leg": "stream_" + k, "frames": SF, "geometry": "512x512 rgb24",
                          "what": "host wall time, VideoHasher() + hash_frame(bytes) per frame + finish()",
                          "median_ms": round(statistics.median(tot), 4), "min_ms": round(min(tot), 4), "max_ms": round(max(tot), 4),
                          "finish_median_ms": round(statistics.median(fin), 4), "finish_min_ms": round(min(fin), 4),
                          "finish_max_ms": round(max(fin), 4), "ratio_to_plain": round(statistics.median(tot) / base, 4),
                          "reps": len(rs)}), flush=True)
    names = ("copy", "submit", "wait")
    us = {}
    for k in names:
        v = C.c_int(0)
        L.check(lib.hvd_debug_get(("hasher_us_" + k).encode(), C.byref(v)))
        us[k] = v.value
    print(json.dumps({"hasher_us_all_legs": us}), flush=True)
