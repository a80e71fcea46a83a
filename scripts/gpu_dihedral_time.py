"""Dihedral PDQ: what the 8 hashes per frame and the mirror/rotation-aware search cost.

1. frames/s of hvd_dev_pdq_hash_frames_dihedral against hvd_dev_pdq_hash_frames, 10 k 64x64 gray frames resident in HBM;
2. the same for 6 144 512x512 rgb24 frames resident in HBM (front-end + hash);
3. seconds per find_transformed_duplicates on a synthetic 100 k-frame library (synth.video_hashes; the non-identity
   variants are further synthetic libraries of the same shape) under "mirror" and "dihedral", against
   find_potential_duplicates.
Device-event timing (hvd_timer_start/stop on the library stream) after warm-up; the search legs also report host wall time.
The clock is the device's rated clock from hvd_runtime_info and, for the search, the FP4-MFMA passes' measured clock.

    python scripts/gpu_dihedral_time.py [--reps 20] [--out dihedral_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import hvd_amd  # noqa: E402
from hvd_amd import _lib as L, synth  # noqa: E402


def event_ms(lib, fn, reps, warmup=3):
    out = []
    for r in range(warmup + reps):
        L.check(lib.hvd_timer_start())
        fn()
        ms = C.c_float(0)
        L.check(lib.hvd_timer_stop(C.byref(ms)))
        if r >= warmup:
            out.append(ms.value)
    return float(np.median(out)), float(np.min(out))


def hash_leg(lib, n, h, w, ch, base, reps):
    """Frames resident in HBM (base tiled up to n), scratch allocated once; plain vs dihedral, same front-end."""
    fb = h * w * ch
    d_f = L.DeviceBuffer(n * fb)
    for f0 in range(0, n, len(base)):
        m = min(len(base), n - f0)
        L.check(lib.hvd_memcpy_h2d(C.c_void_p(d_f.ptr + f0 * fb), base.ctypes.data, m * fb))
    sb = C.c_size_t(0)
    L.check(lib.hvd_pdq_scratch_bytes(n, h, w, ch, C.byref(sb)))
    d_s = L.DeviceBuffer(max(sb.value, 1))
    d_h, d_q = L.DeviceBuffer(n * 256), L.DeviceBuffer(n * 4)
    scr = d_s.ptr if sb.value else None
    plain = event_ms(lib, lambda: L.check(lib.hvd_dev_pdq_hash_frames(d_f.ptr, n, h, w, ch, scr, d_h.ptr, d_q.ptr)), reps)
    h1 = d_h.to_array(np.uint8, n * 32).reshape(n, 32)
    dih = event_ms(lib, lambda: L.check(lib.hvd_dev_pdq_hash_frames_dihedral(d_f.ptr, n, h, w, ch, scr, d_h.ptr, d_q.ptr)),
                   reps)
    h8 = d_h.to_array(np.uint8, n * 256).reshape(n, 8, 32)
    for b in (d_f, d_s, d_h, d_q):
        b.free()
    return {"frames": n, "shape": [h, w, ch], "plain_ms": plain[0], "plain_min_ms": plain[1], "dihedral_ms": dih[0],
            "dihedral_min_ms": dih[1], "plain_fps": n / plain[0] * 1e3, "dihedral_fps": n / dih[0] * 1e3,
            "ratio": dih[0] / plain[0], "variant0_is_plain": bool(np.array_equal(h8[:, 0], h1))}


def search_leg(lib, reps, frames_total=100_000, fpv=64):
    V = frames_total // fpv
    fr, off, _ = synth.video_hashes(V, seed=71, frames_per_video=fpv, copy_fraction=0.02)
    var = {t: synth.video_hashes(V, seed=72 + k, frames_per_video=fpv, copy_fraction=0.0)[0]
           for k, t in enumerate(hvd_amd.vpdq.TRANSFORMS)}
    var["identity"] = fr
    lib_dicts = [{t: var[t][off[v]:off[v + 1]].tobytes() for t in var} for v in range(V)]
    ident = [d["identity"] for d in lib_dicts]
    out = {"videos": V, "frames": int(off[-1])}

    def timed(fn):
        fn()  # warm-up (pools grow, code objects load)
        L.check(lib.hvd_debug_set(b"mfma_clock_reset", 1))
        ev, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            L.check(lib.hvd_timer_start())
            res = fn()
            ms = C.c_float(0)
            L.check(lib.hvd_timer_stop(C.byref(ms)))
            wall.append(time.perf_counter() - t0)
            ev.append(ms.value / 1e3)
        khz = C.c_int(0)
        L.check(lib.hvd_debug_get(b"mfma_pass_khz", C.byref(khz)))
        return {"s": float(np.median(wall)), "event_s": float(np.median(ev)), "pairs": len(res),
                "mfma_pass_mhz": khz.value / 1e3}

    out["plain"] = timed(lambda: hvd_amd.find_potential_duplicates(ident))
    for ts in ("mirror", "dihedral"):
        out[ts] = timed(lambda ts=ts: hvd_amd.find_transformed_duplicates(lib_dicts, transforms=ts))
        out[ts]["ratio"] = out[ts]["s"] / out["plain"]["s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--search-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = L.init(0)
    info = L.runtime_info()
    dev = info.get("devices", [{}])[0]
    res = {"device": dev.get("name"), "arch": dev.get("arch"), "rated_clock_mhz": dev.get("clock_mhz")}
    res["gray64"] = hash_leg(lib, 10000, 64, 64, 1, synth.frames_gray(10000, seed=2), a.reps)
    print(json.dumps(res["gray64"]), flush=True)
    res["rgb512"] = hash_leg(lib, 6144, 512, 512, 3, synth.frames_rgb(64, seed=6), max(3, a.reps // 4))
    print(json.dumps(res["rgb512"]), flush=True)
    res["search"] = search_leg(lib, a.search_reps)
    print(json.dumps(res["search"]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
