"""Times of the bar-colour content rectangle on one MI355X: HIP events on the library stream around each call,
3 warm-up runs, then the median of --reps runs with min..max, the legs interleaved in one process. Frames sit in HBM.
  python scripts/gpu_barcolor_time.py [--reps 15] [--videos 128]
Legs, 512x512 RGB24 as 48-frame videos (6 144 frames by default):
  rects_black   hvd_dev_content_rects on black 64-row bars (init + k_content_rect + finish): the yardstick of DESIGN 4.7
  bar_colors    hvd_dev_bar_colors on white 64-row bars (init + k_corner_fold + finish)
  rects_color   hvd_dev_content_rects_color on them, with the colours bar_colors found (init + k_content_rect_color + finish)
Prints one JSON line per leg and the ratio rects_color / rects_black of the same run."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L  # noqa: E402

HBM_PEAK_TBS = 8.0        # MI355X HBM3E peak
READ_LOOP_TBS = (5.9, 6.15)  # profiles/r05_fetch_calibration.txt: the bare read loop on this class of box

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--videos", type=int, default=128)
args = ap.parse_args()
lib = L.init(0)
H = W = 512
FPV = 48
BARS = 64
V, n = args.videos, args.videos * FPV
rng = np.random.default_rng(1)


def library(white):
    """V videos in HBM: one 48-frame video made on the host, copied V times on the device. Bars: 0..8 (black) or 247..255."""
    one = rng.integers(0, 9, (FPV, H, W, 3), dtype=np.uint8)
    if white:
        one = 255 - one
    one[:, BARS:H - BARS] = rng.integers(40, 216, (FPV, H - 2 * BARS, W, 3), dtype=np.uint8)
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


d_black, d_white = library(False), library(True)
d_off = L.DeviceBuffer.from_array(np.arange(0, n + 1, FPV, dtype=np.int64))
d_rc_b, d_rc_c, d_col = L.DeviceBuffer(16 * V), L.DeviceBuffer(16 * V), L.DeviceBuffer(4 * V)
sb = C.c_size_t(0)
L.check(lib.hvd_bar_colors_scratch_bytes(V, C.byref(sb)))
d_acc = L.DeviceBuffer(sb.value)

legs = {
    "rects_black": lambda: L.check(lib.hvd_dev_content_rects(d_black.ptr, n, H, W, 3, d_off.ptr, V, 16, 1, d_rc_b.ptr)),
    "bar_colors": lambda: L.check(lib.hvd_dev_bar_colors(d_white.ptr, n, H, W, 3, d_off.ptr, V, 16, d_acc.ptr, d_col.ptr)),
    "rects_color": lambda: L.check(lib.hvd_dev_content_rects_color(d_white.ptr, n, H, W, 3, d_off.ptr, V, d_col.ptr, 16, 1,
                                                                   d_rc_c.ptr)),
}
for fn in legs.values():
    fn()
L.check(lib.hvd_dev_sync())
want = (BARS, 0, H - 2 * BARS, W)
assert (d_rc_b.to_array(np.int32, 4 * V).reshape(V, 4) == want).all()
assert (d_rc_c.to_array(np.int32, 4 * V).reshape(V, 4) == want).all()
colours = d_col.to_array(np.int32, V)
assert ((colours & 0xFF) >= 247).all() and ((colours >> 16) >= 247).all()

times = {k: [] for k in legs}
for rep in range(3 + args.reps):
    for k, fn in legs.items():
        ms = timed(fn)
        if rep >= 3:
            times[k].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
nbytes = n * H * W * 3
for k, v in times.items():
    rec = {"leg": k, "frames": n, "videos": V, "geometry": "512x512 rgb24", "what": "call time, HIP events on the library stream",
           "median_ms": round(med[k], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}
    if k != "bar_colors":
        tbs = nbytes / (med[k] * 1e-3) / 1e12
        rec.update(bytes=nbytes, tb_per_s=round(tbs, 3), share_of_read_loop=[round(tbs / x, 3) for x in READ_LOOP_TBS],
                   share_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 3))
    print(json.dumps(rec), flush=True)
print(json.dumps({"ratio": "rects_color / rects_black", "value": round(med["rects_color"] / med["rects_black"], 4),
                  "ranges_disjoint": bool(min(times["rects_color"]) > max(times["rects_black"]))}), flush=True)
for b in (d_black, d_white, d_off, d_rc_b, d_rc_c, d_col, d_acc):
    b.free()
