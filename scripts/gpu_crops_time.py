"""Times of the crop-ladder PDQ path on one MI355X: HIP events on the library stream around each call, 3 warm-ups,
then the median of --reps runs with min..max, the legs interleaved in one process. Frames sit in HBM; nothing outside the
repository is read.
  python scripts/gpu_crops_time.py [--reps 15] [--frames 6144] [--crops aspect]
Legs, 512x512 RGB24:
  crops_fused      hvd_dev_pdq_hash_frames_crops with the whole ladder: the full frame through k_down512w, the K crops in one loop per frame
  separate_sum     the same hashes from the entries that existed before it: one hvd_dev_pdq_hash_frames, then one
                   hvd_dev_pdq_hash_frames_rects per rung with a constant rectangle (one video over all frames); K + 1 reads
  plain            hvd_dev_pdq_hash_frames alone
  rects_<rung>     hvd_dev_pdq_hash_frames_rects with that rung alone
  fused_<rung>     hvd_dev_pdq_hash_frames_crops with that rung alone (K = 1: full frame + rung), against plain + rects_<rung>
Prints one JSON line per leg, then the ratio crops_fused / separate_sum; the new entry must not be slower than the sum."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hvd_amd import _lib as L, vpdq  # noqa: E402

HBM_PEAK_TBS = 8.0        # MI355X HBM3E peak
READ_LOOP_TBS = (5.9, 6.15)  # profiles/r05_fetch_calibration.txt: the bare read loop on this class of box

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--frames", type=int, default=6144)
ap.add_argument("--crops", default="aspect")
args = ap.parse_args()
lib = L.init(0)
H = W = 512
n = args.frames
names, rects = vpdq.crop_ladder(H, W, args.crops)
K = len(names)

# n frames in HBM: 48 random frames made on the host, copied on the device
rng = np.random.default_rng(1)
one = rng.integers(0, 256, (48, H, W, 3), dtype=np.uint8)
d_one = L.DeviceBuffer.from_array(one)
d_fr = L.DeviceBuffer(H * W * 3 * n)
for f0 in range(0, n, 48):
    m = min(48, n - f0)
    L.check(lib.hvd_memcpy_d2d(d_fr.ptr + H * W * 3 * f0, d_one.ptr, H * W * 3 * m))
L.check(lib.hvd_dev_sync())
d_one.free()

sb = C.c_size_t(0)
L.check(lib.hvd_pdq_crops_scratch_bytes(n, H, W, K, C.byref(sb)))
d_cs = L.DeviceBuffer(sb.value)
L.check(lib.hvd_pdq_rects_scratch_bytes(n, H, W, 3, C.byref(sb)))
d_rs = L.DeviceBuffer(sb.value)
d_h8, d_q, d_cq = L.DeviceBuffer(256 * n), L.DeviceBuffer(4 * n), L.DeviceBuffer(32 * n)
d_hs = [L.DeviceBuffer(32 * n) for _ in range(K + 1)]  # the separate entries' hashes, one buffer per rectangle
d_qs = L.DeviceBuffer(4 * n)
d_off = L.DeviceBuffer.from_array(np.array([0, n], dtype=np.int64))
d_rects = [L.DeviceBuffer.from_array(np.ascontiguousarray(r)) for r in rects]


def fused(rung=None):
    rc = rects if rung is None else np.ascontiguousarray(rects[rung:rung + 1])
    L.check(lib.hvd_dev_pdq_hash_frames_crops(d_fr.ptr, n, H, W, 3, rc.ctypes.data, rc.shape[0], d_cs.ptr, d_h8.ptr, d_q.ptr, d_cq.ptr))


def plain():
    L.check(lib.hvd_dev_pdq_hash_frames(d_fr.ptr, n, H, W, 3, d_rs.ptr, d_hs[0].ptr, d_qs.ptr))


def one_rect(k):
    L.check(lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, n, H, W, 3, d_off.ptr, 1, d_rects[k].ptr, d_rs.ptr, d_hs[k + 1].ptr, d_qs.ptr))


def separate():
    plain()
    for k in range(K):
        one_rect(k)


def timed(fn):
    L.check(lib.hvd_timer_start())
    fn()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    return float(ms.value)


# the two routes give the same hashes
fused()
separate()
L.check(lib.hvd_dev_sync())
h8 = d_h8.to_array(np.uint8, 256 * n).reshape(n, 8, 32)
for k in range(K + 1):
    assert np.array_equal(h8[:, k], d_hs[k].to_array(np.uint8, 32 * n).reshape(n, 32)), ("identity",) + names[k - 1:k]
assert not h8[:, K + 1:].any()

legs = {"crops_fused": fused, "separate_sum": separate, "plain": plain}
for k, name in enumerate(names):
    legs[f"rects_{name}"] = lambda k=k: one_rect(k)
    legs[f"fused_{name}"] = lambda k=k: fused(k)
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
    print(json.dumps({"leg": k, "frames": n, "geometry": "512x512 rgb24", "crops": list(names),
                      "what": "call time, HIP events on the library stream", "median_ms": round(med[k], 4),
                      "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v), "frame_bytes": nbytes,
                      "frame_bytes_tb_per_s": round(tbs, 3), "share_of_read_loop": [round(tbs / x, 3) for x in READ_LOOP_TBS],
                      "share_of_hbm_peak": round(tbs / HBM_PEAK_TBS, 3)}), flush=True)
print(json.dumps({"ratio": "crops_fused / separate_sum", "value": round(med["crops_fused"] / med["separate_sum"], 4)}), flush=True)
for k, name in enumerate(names):
    print(json.dumps({"rung": name, "fused_ms": round(med[f"fused_{name}"], 4),
                      "plain_plus_rects_ms": round(med["plain"] + med[f"rects_{name}"], 4)}), flush=True)
for b in [d_fr, d_cs, d_rs, d_h8, d_q, d_cq, d_qs, d_off] + d_hs + d_rects:
    b.free()
