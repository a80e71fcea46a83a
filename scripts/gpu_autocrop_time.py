"""Times of the content-rectangle PDQ path on one MI355X: HIP events on the library stream, warm-up, then the
median of --reps runs with the legs interleaved in one process. Frames sit in HBM.
  python scripts/gpu_autocrop_time.py [--reps 15] [--videos 128] [--small-videos 50000] [--no-pipeline]
Legs, 512x512 RGB24 as 48-frame videos (6 144 frames by default):
  rects_barred        hvd_dev_content_rects on videos with 64-row bars (init + k_content_rect + finish kernels)
  hash_rects_barred   hvd_dev_pdq_hash_frames_rects on them (geometry table, 4 passes per slab, hash kernel)
  hash_generic_full   the generic 4-launch path on the same frames uncropped (pdq_fused_down512 = 0; hvd_dev_pdq_hash_frames)
  plain_unbarred      hvd_dev_pdq_hash_frames on videos without bars (fused kernels)
  auto_unbarred       detection + read-back of the rectangles + hvd_dev_pdq_hash_frames (what the host entry does when every
                      rectangle is full)
  hash_rects_unbarred the rectangle path on full rectangles (what the device-resident entry does)
and rects_small: hvd_dev_content_rects on --small-videos x 64 gray 64x64 frames (no frame is read there: every rectangle is
full by the rule). Prints one JSON line per leg."""
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

HBM_PEAK_TBS = 8.0        # MI355X HBM3E peak
READ_LOOP_TBS = (5.9, 6.15)  # profiles/r05_fetch_calibration.txt: the bare read loop on this class of box

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=128)
ap.add_argument("--small-videos", type=int, default=50000)
ap.add_argument("--no-pipeline", action="store_true")
args = ap.parse_args()
lib = L.init(0)
H = W = 512
FPV = 48
V, n = args.videos, args.videos * FPV
rng = np.random.default_rng(1)


def library(bars):
    """V videos in HBM: one 48-frame video made on the host, copied V times on the device."""
    one = rng.integers(0, 9, (FPV, H, W, 3), dtype=np.uint8)
    one[:, bars:H - bars] = rng.integers(40, 256, (FPV, H - 2 * bars, W, 3), dtype=np.uint8)
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
off = np.arange(0, n + 1, FPV, dtype=np.int64)
d_off = L.DeviceBuffer.from_array(off)
d_rc, d_rc_full = L.DeviceBuffer(16 * V), L.DeviceBuffer(16 * V)
d_h, d_q = L.DeviceBuffer(32 * n), L.DeviceBuffer(4 * n)
sb = C.c_size_t(0)
L.check(lib.hvd_pdq_rects_scratch_bytes(n, H, W, 3, C.byref(sb)))
d_s = L.DeviceBuffer(sb.value)
host_rects = np.zeros((V, 4), np.int32)


def rects(d_fr, d_out):
    L.check(lib.hvd_dev_content_rects(d_fr.ptr, n, H, W, 3, d_off.ptr, V, 16, 1, d_out.ptr))


def hash_rects(d_fr, d_r):
    L.check(lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, n, H, W, 3, d_off.ptr, V, d_r.ptr, d_s.ptr, d_h.ptr, d_q.ptr))


def plain(d_fr, fused=1):
    L.check(lib.hvd_debug_set(b"pdq_fused_down512", fused))
    L.check(lib.hvd_dev_pdq_hash_frames(d_fr.ptr, n, H, W, 3, d_s.ptr, d_h.ptr, d_q.ptr))
    L.check(lib.hvd_debug_set(b"pdq_fused_down512", 1))


def auto_unbarred():
    rects(d_full, d_rc_full)
    L.check(lib.hvd_memcpy_d2h(host_rects.ctypes.data, d_rc_full.ptr, host_rects.nbytes))
    assert (host_rects == (0, 0, H, W)).all()
    plain(d_full)


rects(d_bar, d_rc)
rects(d_full, d_rc_full)
L.check(lib.hvd_dev_sync())
assert (d_rc.to_array(np.int32, 4 * V).reshape(V, 4) == (64, 0, H - 128, W)).all()
legs = {
    "rects_barred": lambda: rects(d_bar, d_rc),
    "hash_rects_barred": lambda: hash_rects(d_bar, d_rc),
    "hash_generic_full": lambda: plain(d_bar, 0),
    "plain_unbarred": lambda: plain(d_full),
    "auto_unbarred": auto_unbarred,
    "hash_rects_unbarred": lambda: hash_rects(d_full, d_rc_full),
}
times = {k: [] for k in legs}
for rep in range(3 + args.reps):
    for k, fn in legs.items():
        ms = timed(fn)
        if rep >= 3:
            times[k].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
nbytes = n * H * W * 3
for k, v in times.items():
    rec = {"leg": k, "frames": n, "geometry": "512x512 rgb24", "what": "call time, HIP events on the library stream",
           "median_ms": round(med[k], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}
    if k == "rects_barred":
        tbs = nbytes / (med[k] * 1e-3) / 1e12
        rec.update(bytes=nbytes, tb_per_s=round(tbs, 3), share_of_read_loop=[round(tbs / x, 3) for x in READ_LOOP_TBS],
                   share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 3))
    print(json.dumps(rec), flush=True)
print(json.dumps({"ratio": "hash_rects_barred / hash_generic_full", "value": round(med["hash_rects_barred"] / med["hash_generic_full"], 4)}))
print(json.dumps({"difference": "auto_unbarred - plain_unbarred", "ms": round(med["auto_unbarred"] - med["plain_unbarred"], 4),
                  "rects_alone_ms": round(med["rects_barred"], 4)}), flush=True)
for b in (d_bar, d_full, d_s, d_h, d_q, d_rc, d_rc_full, d_off):
    b.free()

# ---- many small videos: 64 gray 64x64 frames each ----
SV = args.small_videos
if SV > 0:
    ns = SV * 64
    d_fr = L.DeviceBuffer(ns * 4096)
    L.check(lib.hvd_dev_synth_video_frames(d_fr.ptr, 0, SV, 64, 7, None))
    d_off = L.DeviceBuffer.from_array(np.arange(0, ns + 1, 64, dtype=np.int64))
    d_rc = L.DeviceBuffer(16 * SV)
    ts = [timed(lambda: L.check(lib.hvd_dev_content_rects(d_fr.ptr, ns, 64, 64, 1, d_off.ptr, SV, 16, 1, d_rc.ptr)))
          for _ in range(3 + args.reps)][3:]
    m = statistics.median(ts)
    print(json.dumps({"leg": "rects_small", "videos": SV, "frames": ns, "geometry": "64x64 gray", "median_ms": round(m, 4),
                      "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                      "what": "call time; at 64x64 every rectangle is full by the rule, so no frame is read"}), flush=True)
    for b in (d_fr, d_off, d_rc):
        b.free()

# ---- the chained pipeline on the 30-video library of the tests: stage times ----
if not args.no_pipeline:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import autocrop_helpers as A

    frames, offsets, _, _ = A.library_30()
    d_fr = L.DeviceBuffer.from_array(frames)
    runs = {"autocrop": [], "plain": []}
    for rep in range(2 + 5):
        for name, crop in (("autocrop", True), ("plain", None)):
            tm = {}
            pipeline.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop=crop, timings=tm)
            if rep >= 2:
                runs[name].append(tm)
    for name, rs in runs.items():
        keys = [k for k in ("rects_ms", "hash_ms", "compact_ms", "search_ms") if k in rs[0]]
        print(json.dumps({"pipeline": name, "frames": len(frames), "videos": 30,
                          **{k: round(statistics.median(r[k] for r in rs), 4) for k in keys}}), flush=True)
    d_fr.free()
