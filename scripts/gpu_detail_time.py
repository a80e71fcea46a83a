"""Times of the detail content rectangle on one MI355X: HIP events on the library stream around each call,
3 warm-up runs, then the median of --reps runs with min..max, the legs interleaved in one process. Frames sit in HBM.
  python scripts/gpu_detail_time.py [--reps 15] [--videos 128] > detail_time.jsonl
Legs, 512x512 RGB24 as 48-frame videos (6 144 frames by default) with 64-row blurred bars, both on the same library:
  rects_black    hvd_dev_content_rects (init + k_content_rect + finish): the yardstick of DESIGN 4.7; it finds the full frame
  rects_detail   hvd_dev_content_rects_detail (init + k_content_rect_detail + finish); it finds the 384 rows of picture
Prints one JSON line per leg and the ratio rects_detail / rects_black of the same run. Gray frames, the byte forms and other
geometries are not measured here."""
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


def box_blur(a, axis, radius=24):
    """2 * radius + 1 taps along `axis`: int64 running sum, edge replication."""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    pad = np.concatenate([np.repeat(a[:1], radius, axis=0), a, np.repeat(a[-1:], radius, axis=0)])
    run = np.concatenate([np.zeros_like(pad[:1]), np.cumsum(pad, axis=0)])
    taps = 2 * radius + 1
    return np.moveaxis((run[taps:] - run[:-taps]) // taps, 0, axis)


def library():
    """V videos in HBM: one 48-frame video made on the host, copied V times on the device. Picture: uniform noise in
    40..215 with a slow brightness ramp; bars: the picture's frame blurred three times along both axes and darkened to 3/4."""
    ramp = (np.arange(W) * 40 // W)[None, None, :, None]
    one = (rng.integers(40, 176, (FPV, H, W, 3)) + ramp).astype(np.uint8)
    bg = one.astype(np.int64)
    for _ in range(3):
        bg = box_blur(box_blur(bg, 2), 1)
    bg = (bg * 3 // 4).astype(np.uint8)
    one[:, :BARS] = bg[:, :BARS]
    one[:, H - BARS:] = bg[:, H - BARS:]
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


d_frames = library()
d_off = L.DeviceBuffer.from_array(np.arange(0, n + 1, FPV, dtype=np.int64))
d_rc_b, d_rc_d = L.DeviceBuffer(16 * V), L.DeviceBuffer(16 * V)

legs = {
    "rects_black": lambda: L.check(lib.hvd_dev_content_rects(d_frames.ptr, n, H, W, 3, d_off.ptr, V, 16, 1, d_rc_b.ptr)),
    "rects_detail": lambda: L.check(lib.hvd_dev_content_rects_detail(d_frames.ptr, n, H, W, 3, d_off.ptr, V, 8, 8, d_rc_d.ptr)),
}
for fn in legs.values():
    fn()
L.check(lib.hvd_dev_sync())
assert (d_rc_b.to_array(np.int32, 4 * V).reshape(V, 4) == (0, 0, H, W)).all()
assert (d_rc_d.to_array(np.int32, 4 * V).reshape(V, 4) == (BARS, 0, H - 2 * BARS, W)).all()

times = {k: [] for k in legs}
for rep in range(3 + args.reps):
    for k, fn in legs.items():
        ms = timed(fn)
        if rep >= 3:
            times[k].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
nbytes = n * H * W * 3
for k, v in times.items():
    tbs = nbytes / (med[k] * 1e-3) / 1e12
    print(json.dumps({"leg": k, "frames": n, "videos": V, "geometry": "512x512 rgb24, 64-row blurred bars",
                      "what": "call time, HIP events on the library stream", "median_ms": round(med[k], 4),
                      "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v), "bytes": nbytes,
                      "tb_per_s": round(tbs, 3), "share_of_read_loop": [round(tbs / x, 3) for x in READ_LOOP_TBS],
                      "share_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 3)}), flush=True)
print(json.dumps({"ratio": "rects_detail / rects_black", "value": round(med["rects_detail"] / med["rects_black"], 4),
                  "ranges_disjoint": bool(min(times["rects_detail"]) > max(times["rects_black"])
                                          or max(times["rects_detail"]) < min(times["rects_black"]))}), flush=True)
for b in (d_frames, d_off, d_rc_b, d_rc_d):
    b.free()
