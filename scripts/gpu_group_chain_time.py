"""Time of the grouping on its worst shape, one MI355X: hvd_dev_group_edges over chains -- the records (i, i + s)
of s interleaved paths over L nodes, or a band i ~ i+1..i+w -- whose depth under the rank-less hook rule is the component
until concurrent path halving takes it down. One size and one record order per process:
  python scripts/gpu_group_chain_time.py --nodes 1048576 --order ascending [--stride 1 | --band 3] >> group_chains.jsonl
HIP events on the library stream around the call, one warm-up, the median of --reps runs (min..max); the result is checked once
against the closed form (labels i % s, one group per path; status 1 if it differs). A warm-up call beyond --limit-ms is reported
alone (reps 0); then, or with a median beyond it, the process ends with status 3, so that a caller walking up the sizes stops
there. Prints one JSON line."""
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
from hvd_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, required=True)
ap.add_argument("--order", choices=("ascending", "descending", "shuffled"), default="ascending")
ap.add_argument("--stride", type=int, default=1)
ap.add_argument("--band", type=int, default=0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit-ms", type=float, default=2000.0)
args = ap.parse_args()
V, s = args.nodes, 1 if args.band else args.stride
uv = np.concatenate([np.stack([np.arange(V - d), np.arange(d, V)], axis=1) for d in (range(1, args.band + 1) if args.band else [s])])
if args.order == "descending":
    uv = uv[::-1]
elif args.order == "shuffled":
    uv = np.random.default_rng(V).permutation(uv)
recs = np.zeros(len(uv), dtype=L.PAIR_DTYPE)
recs["i"], recs["j"] = uv[:, 0], uv[:, 1]
E = len(recs)

lib = L.init(0)
sb = C.c_size_t(0)
L.check(lib.hvd_group_scratch_bytes(V, C.byref(sb)))
cap = max(1, s)
d_rec, d_scr, d_label, d_groups, d_cnt = L.DeviceBuffer.from_array(recs), L.DeviceBuffer(sb.value), L.DeviceBuffer(4 * V), \
    L.DeviceBuffer(16 * cap), L.DeviceBuffer(8)


def call():
    L.check(lib.hvd_dev_group_edges(d_rec.ptr, E, None, L.EDGES_ALL, None, 0, 0, V, None, d_scr.ptr, d_label.ptr, d_groups.ptr, cap,
                                    d_cnt.ptr))


def timed():
    L.check(lib.hvd_timer_start())
    call()
    ms = C.c_float(0)
    L.check(lib.hvd_timer_stop(C.byref(ms)))
    return float(ms.value)


L.check(lib.hvd_dev_sync())
t0 = time.perf_counter()
call()
L.check(lib.hvd_dev_sync())
warm_ms = (time.perf_counter() - t0) * 1e3
labels = d_label.to_array(np.int32, V)
groups = d_groups.to_array(L.GROUP_DTYPE, cap)
n = int(d_cnt.to_array(np.uint64, 1)[0])
size = (V - np.arange(s) + s - 1) // s
want = [(r, int(k), (args.band * V - args.band * (args.band + 1) // 2) if args.band else int(k) - 1, r)
        for r, k in enumerate(size.tolist()) if k >= 2]
correct = bool(np.array_equal(labels, np.arange(V) % s)) and n == len(want) and groups[:n].tolist() == want
rec = dict(leg="group_chain", nodes=V, records=E, order=args.order, stride=s, band=args.band, warmup_host_ms=warm_ms, correct=correct)
if warm_ms > args.limit_ms:
    print(json.dumps(dict(rec, reps=0, over_limit_ms=args.limit_ms)), flush=True)
    sys.exit(3)
ms = [timed() for _ in range(args.reps)]
print(json.dumps(dict(rec, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=args.reps, warmup=1)), flush=True)
for b in (d_rec, d_scr, d_label, d_groups, d_cnt):
    b.free()
sys.exit(1 if not correct else 3 if statistics.median(ms) > args.limit_ms else 0)
