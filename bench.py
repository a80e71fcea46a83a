#!/usr/bin/env python
"""bench.py -- headline benchmark of the VPDQ hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: bench.py spawns its own N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W      (any launcher that sets RANK / WORLD_SIZE)

A "step" is one brute-force all-pairs pass (256-bit Hamming, tolerance 31) over a synthetic
hash DB resident in HBM, including the candidate-pair exchange: BASELINE.json configs[2]
(1M hashes, ~5e11 comparisons) at N=1.
  --mode weak   (default) the DB grows so that the comparisons per GPU stay fixed (n = 1M*sqrt(N));
  --mode strong BASELINE configs[2] itself at every N (total work fixed);
  --mode cfg4   BASELINE configs[3]: 10M hashes.
The DB is replicated, tiles of the pair matrix are dealt round-robin to the ranks, the only
collective is the RCCL all-gather of each rank's candidate pairs.

A plain run does only what the headline needs: set up, warm up, time the K steps, write
--dump-outputs, print the line (with the per-step split, the runtime block and the roofline
of the headline's own passes). Everything else runs with --full, in the same run and reported
in the same JSON line: the host re-verification of the headline's pairs, the frame-hashing half
of the metric (configs[1]: 10k pre-decoded 64x64 frames), one pass of configs[3] (10M hashes)
and the chained end-to-end configs[4] (50k videos x 64 frames: hash -> quality filter -> video
search, everything resident in HBM); at N > 1 the strong-scaling companion; at N=1 also the
512x512 RGB24 front-end, the other kernel forms, a CLUSTERED hash DB (the regime of real frame
hashes), a sustained run, the CPU baseline with its oracle gates and the reference-shaped loops.

No PyTorch: the ranks meet over hvd_amd.rendezvous (TCP on loopback; the launcher only provides
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT), the data exchange is RCCL inside the C-ABI.
Rank 0 prints ONE JSON line. The CPU baseline (the oracle, a port -- the reference's real
arithmetic is the absent hvdaccelerators wheel) is timed on rank 0 at N=1 only, with --full.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak (MI355X_MICROARCH.md)
FP4_PEAK_TFLOPS = 10000.0     # dense FP4 MFMA peak (MI355X_MICROARCH.md; measured ceiling 9099)
BYTES_PER_COMPARISON = 64      # two 32-byte operands, no reuse credited
BYTES_PER_FRAME_64 = 4096 + 32 + 4
FLOP_PER_FRAME_64 = 163_840    # the two DCT stages: 2 x 81 920 separately rounded multiplies and adds
VALU_F32_NOFMA_TFLOPS = 78.6   # fp32 VALU peak without FMA (half of the 157.3 TFLOP/s FMA figure, MI355X_MICROARCH.md)
BYTES_PER_FRAME_RGB512 = 786432 + 32 + 4


def host_threads() -> int:
    """Threads for the CPU baseline: os.cpu_count() bounded by the affinity mask and the cgroup CPU quota."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
        except Exception:
            pass
    return max(1, n)


def oracle_check_bands(n, rows_per_block, world=8, seed=46, n_random=32, band_rows=2048):
    """Row bands [(begin, end), ...] (ascending, disjoint) on which the CPU oracle checks an all-pairs result over a DB too
    large to scan whole (BASELINE configs[3], 10M hashes): `n_random` random bands of `band_rows` rows,
    the first and the last rows, and for every rank r a band that straddles the boundary between two row blocks rb-1 | rb
    with (rb + cb_diag) mod world == r for the column chunk holding rb's diagonal -- i.e. the first tile of a row block
    that rank owns. The oracle scans EVERY column j > i for these rows, so each band crosses every column chunk (and with
    it tiles of every rank)."""
    rng = np.random.default_rng(seed)
    starts = [0, max(0, n - band_rows)]
    starts += [int(x) for x in rng.integers(0, max(1, n - band_rows), n_random)]
    n_rb = max(1, (n + rows_per_block - 1) // rows_per_block)
    for r in range(world):
        rb = int(rng.integers(1, max(2, n_rb // world))) * world + r
        if rb < n_rb:
            starts.append(max(0, rb * rows_per_block - band_rows // 2))
    bands = []
    for a in sorted(starts):
        b = min(n, a + band_rows)
        if bands and a < bands[-1][1]:
            bands[-1] = (bands[-1][0], max(bands[-1][1], b))
        else:
            bands.append((a, b))
    return bands


def oracle_hash_device_frames(L, O, d_frames_ptr, n_frames, threads, h=64, w=64, chunk=131072):
    """Read n_frames gray frames back from HBM in chunks and PDQ-hash every one with the CPU oracle (checker of the full-size
    configs[4] test and of bench.py's config5 gate). -> (hashes u8[n,32], quality i32[n])."""
    ho = np.empty((n_frames, 32), dtype=np.uint8)
    qo = np.empty(n_frames, dtype=np.int32)
    fb = h * w
    buf = np.empty((min(chunk, max(1, n_frames)), h, w), dtype=np.uint8)
    for k0 in range(0, n_frames, chunk):
        m = min(chunk, n_frames - k0)
        L.check(L.load().hvd_memcpy_d2h(buf.ctypes.data, C.c_void_p(d_frames_ptr + k0 * fb), m * fb))
        ho[k0:k0 + m], qo[k0:k0 + m] = O.hash_frames(buf[:m], num_threads=threads)
    return ho, qo


def fold_frame_pairs(pairs, video, n_videos, dtype):
    """Host statement of the video-level reduction (vpdqpy/vpdqpy.py:49-56 for every video pair): from frame pairs
    (i < j, frames of different videos, frames stored in video order) to one record per video pair a < b with q_hits =
    distinct frames of a that have a match in b, t_hits = distinct frames of b that have a match in a; sorted by (a, b)."""
    a = video[pairs["i"]].astype(np.int64)
    b = video[pairs["j"]].astype(np.int64)
    assert (a < b).all()  # frames are in video order and pairs inside one video were filtered
    key = a * n_videos + b
    n_fr = np.int64(video.size)
    q = np.unique(key * n_fr + pairs["i"].astype(np.int64)) // n_fr
    t = np.unique(key * n_fr + pairs["j"].astype(np.int64)) // n_fr
    kq, cq = np.unique(q, return_counts=True)
    kt, ct = np.unique(t, return_counts=True)
    assert np.array_equal(kq, kt)
    out = np.zeros(kq.size, dtype=dtype)
    out["a"], out["b"], out["q_hits"], out["t_hits"] = kq // n_videos, kq % n_videos, cq, ct
    return out


MAX_SCLK_MHZ = 2400.0  # MI355X peak engine clock (MI355X_MICROARCH.md): the clock the roofline peaks are quoted at


def gpu_sysfs(pci):
    """Power / clock read-outs of one GPU from sysfs (amdgpu hwmon + pp_dpm_sclk), keyed by its PCI address as
    hvd_runtime_info reports it. Best effort: whatever is not readable on this box (a container without the device's sysfs
    node, another driver) is simply absent; `error` says why when nothing could be read."""
    import glob

    out = {}
    base = None
    want = (pci or "").lower()
    for d in glob.glob("/sys/bus/pci/devices/*"):
        name = os.path.basename(d).lower()
        if want and (name == want or name.endswith(want) or want.endswith(name)):
            base = d
            break
    if base is None:
        cards = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
        if len(cards) == 1:  # a single-GPU box: no need to match the address
            base = os.path.dirname(cards[0])
    if base is None:
        return {"error": f"no sysfs node for PCI device {pci!r}"}

    def read(path):
        try:
            return open(path).read().strip()
        except Exception:
            return None

    for hw in glob.glob(os.path.join(base, "hwmon", "hwmon*")):
        for key, fname, scale in (("power_w", "power1_average", 1e-6), ("power_input_w", "power1_input", 1e-6), ("power_cap_w", "power1_cap", 1e-6),
                                  ("sclk_mhz", "freq1_input", 1e-6), ("mclk_mhz", "freq2_input", 1e-6),
                                  ("temp_c", "temp1_input", 1e-3), ("temp_hotspot_c", "temp2_input", 1e-3)):
            v = read(os.path.join(hw, fname))
            if v is not None:
                try:
                    out[key] = round(float(v) * scale, 1)
                except ValueError:
                    pass
    dpm = read(os.path.join(base, "pp_dpm_sclk"))
    if dpm:
        levels = [ln.strip() for ln in dpm.splitlines()]
        out["pp_dpm_sclk"] = levels
        cur = [ln for ln in levels if ln.endswith("*")]
        if cur:
            try:
                out["dpm_sclk_mhz"] = float(cur[0].split(":")[1].strip().rstrip("*").strip().lower().replace("mhz", ""))
            except Exception:
                pass
    busy = read(os.path.join(base, "gpu_busy_percent"))
    if busy is not None:
        out["gpu_busy_percent"] = busy
    if not out:
        out["error"] = f"nothing readable under {base}"
    return out


class PowerSampler:
    """Background reader of gpu_sysfs() while a leg runs (the sustained leg: the headline's timed steps stay undisturbed)."""

    def __init__(self, pci, period=0.05):
        import threading

        self.pci, self.period, self.samples = pci, period, []
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self._stop.is_set():
            s_ = gpu_sysfs(self.pci)
            if "error" not in s_:
                self.samples.append({k: s_[k] for k in ("power_w", "power_input_w", "sclk_mhz", "dpm_sclk_mhz", "temp_hotspot_c") if k in s_})
            self._stop.wait(self.period)

    def __enter__(self):
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._th.join(2.0)

    def summary(self):
        if not self.samples:
            return {"samples": 0}
        out = {"samples": len(self.samples)}
        for k in self.samples[0]:
            xs = [s_[k] for s_ in self.samples if k in s_]
            if xs:
                out[k] = {"mean": round(float(np.mean(xs)), 1), "min": min(xs), "max": max(xs)}
        return out


def pass_clock_mhz(lib, L):
    """Effective shader clock (MHz) of this context's FP4-MFMA all-pairs passes since the last reset (in-kernel s_memtime /
    s_memrealtime brackets of one workgroup in eight: include/hvd_mi355x.h "mfma_pass_khz"), and the number of samples."""
    khz, ns = C.c_int(0), C.c_int(0)
    L.check(lib.hvd_debug_get(b"mfma_pass_khz", C.byref(khz)))
    L.check(lib.hvd_debug_get(b"mfma_clock_samples", C.byref(ns)))
    return (khz.value / 1e3 if khz.value > 0 else None), ns.value


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=("weak", "strong", "cfg4"), default="weak")
    ap.add_argument("--hashes", type=int, default=1_000_000, help="DB size at N=1 (weak/strong modes)")
    ap.add_argument("--frames", type=int, default=10_000)
    ap.add_argument("--variant", type=int, default=-1, help="all-pairs kernel variant (-1: product default)")
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg and gate (frames hashed, configs[3] / configs[4], strong scaling, kernel forms, "
                         "clustered DBs, RGB24, streaming feeds, sustained, CPU baseline + oracle gates, reference-shaped loops); "
                         "default: the headline alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and its oracle gates")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--oracle-check-seconds", type=float, default=90.0,
                    help="budget (estimated CPU seconds) of EACH full-size oracle gate of the cpu_baseline leg (config4 row bands, "
                         "config5 every frame + every frame pair); a gate whose estimate exceeds it is skipped with the reason")
    ap.add_argument("--sustain-seconds", type=float, default=12.0, help="length of the sustained leg at N=1 with --full (0: skip)")
    ap.add_argument("--no-extras", action="store_true", help="--full: headline + frames_hashed only")
    ap.add_argument("--cfg5-videos", type=int, default=50_000)
    ap.add_argument("--single-process", action="store_true",
                    help="N > 1 inside ONE process: the library's device group (hvd_init_devices, ncclCommInitAll), one "
                         "thread per GPU -- the mode the drop-in surfaces use (HVD_DEVICES); default: one process per GPU")
    ap.add_argument("--devices", type=str, default="", help="--single-process: comma-separated device list (default 0..N-1; "
                                                             "a device may be listed twice: host-memory exchange)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write the headline's pair list of the last step to DIR/pairs_{i,j,dist}.npy "
                         "(float64, sorted by (i, j); a seeded sample of rows if it exceeds 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, merged):
    """The headline's result as its caller receives it (hvd_amd.allpairs_hamming: records (i, j, dist) sorted by (i, j)),
    one float64 array per field. Over DUMP_LIMIT_BYTES, a fixed seeded sample of the records, kept in (i, j) order."""
    fields = ("i", "j", "dist")
    rows = np.arange(merged.size)
    max_rows = DUMP_LIMIT_BYTES // (8 * len(fields))
    if rows.size > max_rows:
        rows = np.sort(np.random.default_rng(0).choice(rows, size=max_rows, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    for f in fields:
        np.save(os.path.join(out_dir, f"pairs_{f}.npy"), merged[f][rows].astype(np.float64))
    return {"dir": out_dir, "records": int(merged.size), "records_written": int(rows.size),
            "arrays": [f"pairs_{f}.npy" for f in fields]}


def mean_sd(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return float(xs.mean()), float(xs.std(ddof=1)) if xs.size > 1 else 0.0


def sig(x, digits=4):
    return float(f"{x:.{digits}g}")


TRAFFIC_SOURCE = ("profiles/hbm_traffic.json: PMC bytes per launch from a separate rocprofv3 --pmc side-run of the same "
                  "kernels (FETCH_SIZE x2 + WRITE_SIZE, separate passes), not re-measured inside this run")


def k1_roofline(fps_per_gpu, traffic):
    """64x64 hash kernel: bound by the fp32 VALU (the bit-exact DCT is 2 separately rounded ops per MAC, no FMA, no
    MFMA), so the fraction is executed DCT flop over the non-FMA fp32 peak; the HBM view rides along."""
    tf = fps_per_gpu * FLOP_PER_FRAME_64 / 1e12
    gbs = fps_per_gpu * BYTES_PER_FRAME_64 / 1e9
    return {"bound": "valu", "kernel": "k_pdq_hash64", "achieved": round(tf, 2), "peak": VALU_F32_NOFMA_TFLOPS,
            "unit": "TFLOP/s", "frac": round(tf / VALU_F32_NOFMA_TFLOPS, 3), "traffic": traffic,
            "traffic_source": TRAFFIC_SOURCE if traffic is not None else None,
            "hbm": {"achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4)},
            "note": "algorithmic flop = 163 840 per frame (the two DCT stages, multiply and add rounded separately); "
                    "algorithmic bytes = 4 132 per frame; peak = fp32 VALU without FMA"}


def load_traffic(key):
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json"))).get(key)
    except Exception:
        return None


def traffic_provenance():
    """Is profiles/hbm_traffic.json still about THESE kernels? The file records the sha256 of the kernel sources it was measured
    on (scripts/make_hbm_traffic.py); a kernel file that has changed since makes every `traffic` of this line stale."""
    import hashlib

    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
        want = rec.get("_kernel_sources_sha256") or {}
        csrc = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
        changed = sorted(f for f, h in want.items()
                         if hashlib.sha256(open(os.path.join(csrc, f), "rb").read()).hexdigest()[:16] != h)
        return {"measured_in": rec.get("_round"), "kernel_sources_changed_since": changed, "stale": bool(changed) or not want}
    except Exception as exc:  # noqa: BLE001
        return {"stale": True, "error": repr(exc)}


def videohasher_stream_leg(lib, L, synth, vpdq):
    """The reference's actual hashing call pattern (vpdqpy/vpdqpy.py:113-119): ONE VideoHasher per video, one
    hash_frame(...) per frame, finish() per video, videos strictly one after the other -- through the drop-in Python
    class, host frames in, VpdqHash out, PCIe and every Python call inside the timed region. Four feeds:
      bytes         hash_frame(bytes)            what the unchanged reference loop passes (a 786 KB memcpy into the ring)
      buffer        hash_frame(ndarray row)      any buffer object, same memcpy, no bytes object
      acquire_copy  acquire_frame() + np.copyto + commit_frame()   a decoder writing at memcpy speed into the pinned slot
      acquire_only  acquire_frame() + commit_frame()               the feed's own ceiling: nothing is written, the slots keep what
                                                                   a warm-up video wrote (a video of ONE repeated frame, so that
                                                                   every slot position holds it whatever the batch layout)
      acquire_run   acquire_frames(k) + ONE np.copyto per run + commit_frames()   a decoder that fills a run of frames per call
      bytes_memcpy  hash_frame(bytes) with the ring copy as plain memcpy (hvd_debug_set copy_nt 0): the A/B of the
                    non-temporal stores the copy slices use by default (round 5)
    Every video's hash is compared with the batch entry point's. Next to it: a pinned host->device bandwidth probe taken
    in the same run; `h2d_frac` = frame bytes/s over that probe."""
    out = {}
    nb = 256 << 20
    hp = C.c_void_p()
    L.check(lib.hvd_host_malloc(C.byref(hp), nb))
    C.memset(hp, 1, nb)
    d = L.DeviceBuffer(nb)
    rates = []
    for _ in range(7):
        t = time.perf_counter()
        L.check(lib.hvd_memcpy_h2d(d.ptr, hp, nb))
        rates.append(nb / (time.perf_counter() - t) / 1e9)
    d.free()
    L.check(lib.hvd_host_free(hp))
    h2d = float(np.median(rates[1:]))
    out["h2d_probe"] = {"GBps": round(h2d, 2), "GBps_best": round(max(rates), 2),
                        "what": "256 MiB hipMemcpy from page-locked host memory (hvd_host_malloc), median of 6"}
    frames_per_video = 300
    for name, (w, h, ch, n_videos) in (("512x512_rgb24", (512, 512, 3, 12)), ("64x64_gray", (64, 64, 1, 60))):
        if ch == 3:
            distinct = synth.frames_rgb(16, seed=6)
        else:
            distinct = synth.frames_gray(frames_per_video, seed=2)
        video = np.ascontiguousarray(distinct[np.arange(frames_per_video) % distinct.shape[0]])
        hh, qq = vpdq.hash_frames(video)
        want = hh[qq >= 31].tobytes()
        fb = video[0].nbytes
        as_bytes = [video[k].tobytes() for k in range(frames_per_video)]
        rows = video.reshape(frames_per_video, -1)
        res = {"frames_per_video": frames_per_video, "videos": n_videos, "frame_bytes": fb,
               "frames_kept_per_video": len(want) // 32}

        same = np.ascontiguousarray(np.broadcast_to(distinct[:1], video.shape))  # acquire_only: one frame, repeated
        hs_, qs_ = vpdq.hash_frames(same[:1])
        want_same = (hs_[:1].tobytes() * frames_per_video) if qs_[0] >= 31 else b""

        def run(feed, video=video):
            hs = vpdq.VideoHasher(1, w, h, 0)
            if feed == "bytes":
                for f in as_bytes:
                    hs.hash_frame(f)
            elif feed == "buffer":
                for k in range(frames_per_video):
                    hs.hash_frame(rows[k])
            elif feed == "acquire_copy":
                for k in range(frames_per_video):
                    np.copyto(hs.acquire_frame(ch), video[k])
                    hs.commit_frame()
            elif feed == "acquire_run":
                k = 0
                while k < frames_per_video:
                    run_ = hs.acquire_frames(frames_per_video - k, ch)
                    np.copyto(run_, video[k:k + run_.shape[0]])
                    hs.commit_frames()
                    k += run_.shape[0]
            else:
                for k in range(frames_per_video):
                    hs.acquire_frame(ch)
                    hs.commit_frame()
            return hs.finish()

        nt_level = C.c_int(0)
        L.check(lib.hvd_debug_get(b"copy_nt", C.byref(nt_level)))
        res["copy_nt_level"] = {0: "plain memcpy", 2: "AVX2 streaming stores", 3: "AVX-512 streaming stores"}.get(nt_level.value, "?")
        # Three interleaved rounds over the feeds, the MEDIAN round reported per feed (with the spread): one round is 12 videos
        # = 60 ms per feed, and single rounds of this host-side pipeline scatter by +-10 % (page placement, the other legs'
        # leftovers, clocks) -- more than the differences between the feeds.
        feeds = [f_ for f_ in ("bytes", "bytes_memcpy", "buffer", "acquire_only", "acquire_copy", "acquire_run")
                 if not (f_ == "bytes_memcpy" and (ch != 3 or nt_level.value == 0))]
        rounds = {f_: [] for f_ in feeds}
        for rnd in range(3):
            for feed in feeds:  # (fast feeds first)
                if feed == "bytes_memcpy":
                    L.check(lib.hvd_debug_set(b"copy_nt", 0))
                real = "bytes" if feed == "bytes_memcpy" else feed
                if feed == "acquire_only":
                    assert run("acquire_copy", same).bytes == want_same  # warm-up: every slot position now holds that frame
                    expect = want_same
                else:
                    assert run(real).bytes == want  # warm-up
                    expect = want
                t_w = time.perf_counter()  # 0.2 s (first round; then 0.05 s) of untimed videos of the feed itself: after a pause or a slow
                while time.perf_counter() - t_w < (0.2 if rnd == 0 else 0.05):  # leg the first videos of a fast feed ran up to 40 % slower
                    run(real)                                                    # (clocks / DMA state): an artefact of the order of the legs
                t = time.perf_counter()
                for _ in range(n_videos):
                    got = run(real)
                    assert got.bytes == expect, f"VideoHasher({feed}) differs from the batch entry point"
                rounds[feed].append(time.perf_counter() - t)
                if feed == "bytes_memcpy":
                    L.check(lib.hvd_debug_set(b"copy_nt", 1))
        for feed in feeds:
            dts = sorted(rounds[feed])
            dt = dts[len(dts) // 2]
            fps = n_videos * frames_per_video / dt
            res[feed] = {"frames_per_s": sig(fps), "GBps": round(fps * fb / 1e9, 2), "h2d_frac": round(fps * fb / 1e9 / h2d, 3),
                         "ms_per_video": round(dt / n_videos * 1e3, 3), "us_per_frame": round(dt / n_videos / frames_per_video * 1e6, 2),
                         "rounds_us_per_frame": [round(x / n_videos / frames_per_video * 1e6, 2) for x in rounds[feed]]}
        res["rounds"] = "3 interleaved rounds of %d videos per feed; the median round is reported, `rounds_us_per_frame` lists all three" % n_videos
        out[name] = res
    return out


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` with no launcher environment: spawn the N ranks ourselves (one process per
    GPU: RANK = LOCAL_RANK = r, WORLD_SIZE = N, a free MASTER_PORT, a private rendezvous file), forward rank 0's
    single JSON line, return non-zero if ANY rank fails (the others are then terminated, not left hanging in a
    barrier). No torch anywhere; `python -m torch.distributed.run ... bench.py` keeps working as before."""
    import shutil
    import socket
    import subprocess
    import tempfile

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    rdzv_dir = tempfile.mkdtemp(prefix="hvd_bench_")  # 0700, ours alone
    base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                HVD_RDZV_FILE=os.path.join(rdzv_dir, "rdzv"))
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = []
    try:
        for r in range(n):
            env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr))
        import threading

        box = {}
        reader = threading.Thread(target=lambda: box.setdefault("out", procs[0].stdout.read()), daemon=True)
        reader.start()
        rcs = [None] * n
        failed = None
        while any(rc is None for rc in rcs):
            for r, p in enumerate(procs):
                if rcs[r] is None:
                    rcs[r] = p.poll()
                    if rcs[r] not in (None, 0) and failed is None:
                        failed = r
            if failed is not None:
                break
            time.sleep(0.05)
        if failed is not None:
            print(f"[bench] rank {failed} exited with {rcs[failed]}; terminating the other ranks", file=sys.stderr)
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            for p in procs:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()
            return rcs[failed] if rcs[failed] > 0 else 1
        reader.join(timeout=10)
        lines = [ln for ln in (box.get("out") or b"").decode().splitlines() if ln.startswith("{")]
        if len(lines) != 1:
            print(f"[bench] rank 0 printed {len(lines)} JSON lines (expected 1)", file=sys.stderr)
            return 1
        sys.stdout.write(lines[0] + "\n")
        sys.stdout.flush()
        return 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        shutil.rmtree(rdzv_dir, ignore_errors=True)


def main():
    args = parse()
    if args.single_process and args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(single_process(args))
    if "RANK" not in os.environ and "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args.gpus))
    # Native libraries (RCCL) print banners on fd 1; the contract is ONE JSON line on stdout.
    # Keep the real stdout aside and point fd 1 at stderr for everything else.
    sys.stdout.flush()
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world  # a launcher's WORLD_SIZE wins over the flag
    rank_main(args, rank, local_rank, world, real_stdout, None)


def single_process(args) -> int:
    """`python bench.py --gpus N --single-process`: the N ranks are the N contexts of the library's in-process device group
    (hvd_init_devices: one stream / pool / communicator per device, ncclCommInitAll), each driven by one thread of this
    process -- what a hydrus user gets from HVD_DEVICES=0,1,...; same workloads, same JSON line, `"launch": "single-process"`."""
    import threading

    sys.stdout.flush()
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    from hvd_amd import _lib as L
    from hvd_amd.rendezvous import ThreadRendezvous

    if L.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    devs = [int(d) for d in args.devices.split(",")] if args.devices else list(range(args.gpus))
    if len(devs) != args.gpus:
        raise SystemExit(f"--devices lists {len(devs)} devices, --gpus says {args.gpus}")
    L.init_devices(devs)
    members = ThreadRendezvous.group(args.gpus)
    failed = []

    def body(r):
        try:
            L.set_context(r)
            rank_main(args, r, r, args.gpus, real_stdout, members[r])
        except BaseException as exc:  # noqa: BLE001 - any rank's failure fails the run (and must not strand the others)
            import traceback

            traceback.print_exc()
            failed.append((r, repr(exc)))
            members[r].abort()
            L.group_abort()

    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(1, args.gpus)]
    for t in ts:
        t.start()
    body(0)
    for t in ts:
        t.join(600)
    return 1 if failed or any(t.is_alive() for t in ts) else 0


def rank_main(args, rank, local_rank, world, real_stdout, inproc):
    """One rank of the bench: a process of its own (inproc is None: the default) or one thread of `--single-process`
    (inproc = this rank's ThreadRendezvous; the library's current context is already this rank's)."""
    import hvd_amd
    from hvd_amd import _lib as L
    from hvd_amd import multigpu as M
    from hvd_amd import pipeline, search, synth
    from hvd_amd.rendezvous import Rendezvous

    # The line's `policies` block already states the comparator left at its default; the library's one-time warning about
    # it would reach stderr while the reference-shaped legs run and end the run's output after the JSON line.
    warnings.filterwarnings("ignore", message="hvd_amd: frame comparator left at its default", category=RuntimeWarning)
    ndev = L.device_count()
    if ndev < 1:
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    exchange, host_ex = None, None
    exchange_kind = "none"
    hard_exit = False  # a bootstrap thread stuck inside RCCL cannot be joined: leave with os._exit
    if inproc is not None:
        lib = L.load()
        rdzv = inproc
        if world > 1:
            exchange = M.GroupExchange(rank, world)
            exchange_kind = "rccl" if L.group_exchange() == "rccl" else "host-memory (in-process group without RCCL: a device listed twice)"
    else:
        # one process per GPU: LOCAL_RANK picks the device; if the launcher masks devices per rank
        # (HIP_VISIBLE_DEVICES), every rank sees a single device 0. HVD_FORCE_DEVICE: dev testing only.
        dev = int(os.environ.get("HVD_FORCE_DEVICE", local_rank if local_rank < ndev else local_rank % ndev))
        lib = L.init(dev)
        rdzv = Rendezvous(rank, world)
    if world > 1 and inproc is None:
        # ncclCommInitRank is collective and bounded, so that a hung bootstrap degrades to exchanging the candidates
        # over the control channel (reported in the JSON) instead of producing no measurement at all.
        exchange, why, hard_exit = M.connect_rccl(rdzv, float(os.environ.get("HVD_RCCL_INIT_TIMEOUT", "120")))
        if exchange is not None:
            # the communicator exists; can it move data? One 16-byte all-gather under a deadline decides for all ranks.
            ok, why, stuck = M.preflight_rccl(rdzv, exchange, float(os.environ.get("HVD_RCCL_PREFLIGHT_TIMEOUT", "60")))
            if not ok:
                hard_exit = hard_exit or stuck
                # ncclCommAbort also unblocks a collective that hangs on the device (it sits on the library stream, which
                # the kernels need); bounded, because nothing here may be able to hang the measurement
                import threading

                ab = threading.Thread(target=lambda: exchange.abort(), daemon=True)
                ab.start()
                ab.join(30.0)
                hard_exit = hard_exit or ab.is_alive()
                exchange = None
                why = "preflight all-gather " + why
        if exchange is not None:
            exchange_kind = "rccl"
        else:
            print(f"[bench] rank {rank}: RCCL init {why}; exchanging candidates over TCP", file=sys.stderr)
            host_ex = M.HostExchange(rdzv)
            exchange_kind = "tcp-fallback"

    def barrier():
        # the kernels run on the library's own HIP stream; hipDeviceSynchronize (every stream of this rank's GPU,
        # RCCL's included) is the counterpart of torch.cuda.synchronize()
        L.check(lib.hvd_device_synchronize())
        rdzv.barrier()

    variant = search.DEFAULT_VARIANT if args.variant < 0 else args.variant
    # the semantics the absent wheel leaves open: every artefact carries the labels
    policies = hvd_amd.vpdq.policy_labels()
    # what the ranks run on: versions, library paths, every rank's device, the peer links between them (xGMI or PCIe)
    try:
        runtime = L.runtime_info()
    except Exception as exc:  # noqa: BLE001 - a diagnostics block must not be able to take the measurement with it
        runtime = {"error": repr(exc)}
    runtime.setdefault("devices", [])
    runtime.setdefault("visible_devices", ndev)
    my_dev = local_rank if inproc is not None else int(os.environ.get("HVD_FORCE_DEVICE", local_rank if local_rank < ndev else local_rank % ndev))
    my_pci = next((d_["pci"] for d_ in runtime["devices"] if d_["index"] == my_dev), "?")
    runtime["ranks"] = [json.loads(p_) for p_ in rdzv.allgather(json.dumps(
        {"rank": rank, "device": my_dev, "pid": os.getpid(),
         "pci": my_pci,
         "visible": os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES", ""))}).encode())]
    links = sorted({p_["link"] for p_ in runtime.get("peers", [])})
    runtime["xgmi_or_pcie"] = "/".join(links) if links else ("single device" if runtime["visible_devices"] <= 1 else "?")
    runtime["exchange"] = exchange_kind
    runtime["group_exchange"] = L.group_exchange() if inproc is not None else "n/a (one process per GPU)"

    # ---------------- headline workload: replicated synthetic hash DB ---------------------------
    if args.mode == "cfg4":
        n, seed, scaling = 10_000_000, 4, "strong"
        wl = "BASELINE configs[3]: 10M hashes"
    elif args.mode == "strong" or world == 1:
        n, seed, scaling = args.hashes, 3, ("weak" if world == 1 else "strong")
        wl = "BASELINE configs[2]" if n == 1_000_000 else f"configs[2] shape at n={n}"
    else:
        n, seed, scaling = int(round(args.hashes * math.sqrt(world) / 1024.0)) * 1024, 3, "weak"
        wl = f"configs[2] scaled weakly: n = {args.hashes}*sqrt({world})"

    def allpairs_workload(n_, seed_, steps, warmup, v=variant, db_=None, planted_=None, cap=1 << 20, verify=True):
        """K timed steps (FP4 image + all-pairs pass over this rank's tiles + pair read-back + exchange)."""
        if db_ is None:
            db_, planted_ = synth.hash_db(n_, seed=seed_)
        d_db = L.DeviceBuffer.from_array(db_)
        img_bytes = C.c_size_t(0)
        L.check(lib.hvd_fp4_image_bytes(n_, C.byref(img_bytes)))
        d_img = L.DeviceBuffer(img_bytes.value)
        d_pairs = L.DeviceBuffer(16 * cap)
        d_cnt = L.DeviceBuffer(8)
        kms, my_pairs = [], [0]
        # per timed step, on this rank (the first multi-GPU run must be readable from its one JSON line):
        #   expand_ms   FP4 image of the DB (HIP events on the library stream)
        #   kernel_ms   probe + form selection + all-pairs kernel over this rank's tiles (HIP events)
        #   readback_ms pair count + this rank's records device -> host (host clock, after the kernel has finished)
        #   exchange_ms the candidate exchange (RCCL all-gather of counts and padded records incl. their read-back; TCP in the
        #               fallback; 0 at N = 1)
        #   host_ms     the rest of the step's wall time: Python, ctypes, launch latency, the memset of the counter
        split = {k: [] for k in ("expand_ms", "kernel_ms", "readback_ms", "exchange_ms", "host_ms", "step_ms")}

        def between(a, b):
            ms = C.c_float(0)
            L.check(lib.hvd_timer_between(a, b, C.byref(ms)))
            return float(ms.value)

        def step(timed=True):
            t_a = time.perf_counter()
            d_cnt.zero()
            L.check(lib.hvd_timer_mark(0))
            if v >= 8:  # the FP4 image is rebuilt inside every step: it is part of the pass, not a cached index
                L.check(lib.hvd_dev_expand_fp4(d_db.ptr, n_, d_img.ptr))
            L.check(lib.hvd_timer_mark(1))
            M.launch_allpairs(lib, d_db.ptr, d_img.ptr, n_, None, 31, rank, world, d_pairs.ptr, cap, d_cnt.ptr, v)
            L.check(lib.hvd_timer_mark(2))
            L.check(lib.hvd_dev_sync())  # the pass has finished on the device
            t_k = time.perf_counter()
            cnt = int(d_cnt.to_array(np.uint64, 1)[0])
            if cnt > cap:
                raise RuntimeError("pair buffer overflow in bench")
            my_pairs[0] = cnt
            if world == 1:
                out_ = d_pairs.to_array(L.PAIR_DTYPE, cnt)
                t_r = t_x = time.perf_counter()
            elif exchange is not None:
                t_r = time.perf_counter()
                out_ = exchange.allgather_pairs_dev(d_pairs.ptr, cnt)
                t_x = time.perf_counter()
            else:
                mine_ = d_pairs.to_array(L.PAIR_DTYPE, cnt)
                t_r = time.perf_counter()
                out_ = host_ex.allgather_pairs(mine_)
                t_x = time.perf_counter()
            if timed:
                e_ms, k_ms = between(0, 1), between(1, 2)
                kms.append(k_ms)
                r_ms, x_ms, s_ms = (t_r - t_k) * 1e3, (t_x - t_r) * 1e3, (t_x - t_a) * 1e3
                for key, val in (("expand_ms", e_ms), ("kernel_ms", k_ms), ("readback_ms", r_ms), ("exchange_ms", x_ms),
                                 ("host_ms", s_ms - e_ms - k_ms - r_ms - x_ms), ("step_ms", s_ms)):
                    split[key].append(round(val, 3))
            return out_

        for _ in range(warmup):
            step(timed=False)
        if v >= 8:
            L.check(lib.hvd_debug_set(b"mfma_clock_reset", 1))  # (enqueued in stream order; read after the timed region)
        sys_before = gpu_sysfs(my_pci)
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            recs = step()
        barrier()
        elapsed = rdzv.allreduce_max([time.perf_counter() - t0])[0]
        sys_after = gpu_sysfs(my_pci)
        clk_mhz, clk_samples = pass_clock_mhz(lib, L) if v >= 8 else (None, 0)
        merged = M.merge_pairs([recs])
        if verify:
            # parity gate that runs with every measurement of --full: every reported pair verifies on the host with its
            # exact distance, and every planted pair within tolerance is reported
            dist_host = np.unpackbits(db_[merged["i"]] ^ db_[merged["j"]], axis=1).sum(1)
            assert np.array_equal(dist_host, merged["dist"]) and (merged["dist"] <= 31).all()
            if planted_ is not None and len(planted_):
                d_pl = np.unpackbits(db_[planted_[:, 0]] ^ db_[planted_[:, 1]], axis=1).sum(1)
                want = {(int(min(s, d)), int(max(s, d))) for (s, d, _), dd in zip(planted_, d_pl) if dd <= 31}
                assert want <= set(zip(merged["i"].tolist(), merged["j"].tolist())), "planted duplicate pair missed"
        # every rank must hold the identical merged pair list after the exchange
        digest = int(np.bitwise_xor.reduce(merged.view(np.uint32).astype(np.uint64) *
                                           np.arange(1, merged.size * 4 + 1, dtype=np.uint64))) if merged.size else 0
        per_rank = rdzv.allgather(json.dumps({"rank": rank, "kernel_ms": round(float(np.mean(kms)), 3),
                                              "effective_mhz": round(clk_mhz, 1) if clk_mhz else None, "clock_samples": clk_samples,
                                              "sysfs_before": sys_before, "sysfs_after": sys_after,
                                              **{k_: round(float(np.mean(v_)), 3) for k_, v_ in split.items() if k_ != "kernel_ms"},
                                              "pairs": my_pairs[0], "merged_pairs": int(merged.size), "digest": digest,
                                              "steps": split}).encode())
        if verify:
            assert len({(json.loads(p)["merged_pairs"], json.loads(p)["digest"]) for p in per_rank}) == 1, \
                "ranks disagree on the merged pair list"
        res = {"elapsed": elapsed, "kernel_ms": kms, "merged": merged, "per_rank": [json.loads(p) for p in per_rank],
               "bufs": (d_db, d_img, d_pairs, d_cnt), "db": db_}
        return res

    # ---------------- frames hashed / s (BASELINE configs[1]), every rank hashes its own batch ----
    K1_WARM = 20

    def time_k1(nf, reps):
        fr_ = synth.frames_gray(min(nf, 10_000), seed=2)
        d_f = L.DeviceBuffer(nf * 4096)
        for r0 in range(0, nf, fr_.shape[0]):  # larger batches replicate the 10k distinct frames on the device
            m = min(fr_.shape[0], nf - r0)
            L.check(lib.hvd_memcpy_h2d(C.c_void_p(d_f.ptr + r0 * 4096), fr_.ctypes.data, m * 4096))
        d_h, d_q = L.DeviceBuffer(32 * nf), L.DeviceBuffer(4 * nf)
        for _ in range(K1_WARM):  # untimed: the clocks settle over the first launches after a host-side pause
            L.check(lib.hvd_dev_pdq_hash_frames(d_f.ptr, nf, 64, 64, 1, None, d_h.ptr, d_q.ptr))
        barrier()
        ks = []
        t0 = time.perf_counter()
        for _ in range(reps):
            L.check(lib.hvd_timer_start())
            L.check(lib.hvd_dev_pdq_hash_frames(d_f.ptr, nf, 64, 64, 1, None, d_h.ptr, d_q.ptr))
            ms = C.c_float(0)
            L.check(lib.hvd_timer_stop(C.byref(ms)))
            ks.append(ms.value)
        barrier()
        wall = time.perf_counter() - t0
        d_f.free()
        return fr_, d_h, d_q, ks, wall

    # what runs besides the headline: with --full the frames_hashed leg, and unless --no-extras every other leg and gate
    full_legs = args.full and not args.no_extras

    # --full: the 64x64 hash leg once BEFORE the matrix-core workload (chip idle until now) and once after it (below: the
    # reported `value`): after 0.5 s of FP4 MFMAs at the power limit the clocks are lower for a while, and 10k frames take 50 us
    if args.full:
        _, dh0, dq0, k1_idle, _ = time_k1(args.frames, 50)
        dh0.free()
        dq0.free()
        k1_idle_ms = rdzv.allreduce_max([mean_sd(k1_idle)[0]])[0]

    total_cmp = n * (n - 1) // 2
    head = allpairs_workload(n, seed, args.steps, args.warmup, verify=args.full)
    form = variant
    if variant == 13:  # which of its two forms did the probe choose for this DB? (read before any other leg launches)
        fv = C.c_int(0)
        L.check(lib.hvd_debug_get(b"mfma_auto_form", C.byref(fv)))
        form = fv.value
    d_db, d_img, d_pairs, d_cnt = head["bufs"]
    db = head["db"]
    elapsed, merged = head["elapsed"], head["merged"]
    dumped = dump_outputs(args.dump_outputs, merged) if args.dump_outputs and rank == 0 else None
    kernel_avg_ms = max(p["kernel_ms"] for p in head["per_rank"])  # the slowest rank's mean launch duration
    k_mean, k_sd = mean_sd(head["kernel_ms"])
    ms_per_step = elapsed / args.steps * 1e3
    value = total_cmp / (elapsed / args.steps)

    # --full, N > 1 in the default (weak) mode: BASELINE configs[2] itself -- fixed total work -- in the same run, so that one
    # driver run per N yields both scaling curves
    strong = None
    if full_legs and world > 1 and args.mode == "weak":
        k_s = max(1, min(args.steps, 10))
        rs = allpairs_workload(args.hashes, 3, steps=k_s, warmup=1)
        for b in rs["bufs"]:
            b.free()
        tc_s = args.hashes * (args.hashes - 1) // 2
        strong = {"workload": f"BASELINE configs[2]: {args.hashes} hashes at every N (fixed total work), {k_s} timed steps",
                  "value": sig(tc_s / (rs["elapsed"] / k_s), 5), "unit": "comparisons/s", "scaling": "strong", "n_gpus": world,
                  "ms_per_step": round(rs["elapsed"] / k_s * 1e3, 3), "steps": k_s, "warmup": 1,
                  "pairs_found": int(len(rs["merged"])), "per_rank": rs["per_rank"]}
        del rs

    if args.full:
        fr, d_h, d_q, k1_list, k1_wall = time_k1(args.frames, 50)
        k1_ms, k1_sd = mean_sd(k1_list)
        k1_ms, k1_wall = rdzv.allreduce_max([k1_ms, k1_wall])

    # ---------------- BASELINE configs[3] (10M hashes) and configs[4] (end to end), at every N --------------
    # At N > 1 these two legs run paths that a 1-GPU development box cannot exercise (RCCL all-gathers of hash shards and
    # key sets between real ranks). They must not be able to take the headline measurement with them: they run under a
    # deadline (HVD_BENCH_EXTRAS_TIMEOUT seconds, default 600); on an exception or a hang the JSON line is still printed,
    # with the reason in place of the leg, and the process leaves with os._exit (a rank stuck in a collective cannot be
    # joined).
    extras = {}
    # the full-size oracle gates of the cpu_baseline leg (below) need what these legs produced: kept on the host / in HBM until then
    want_oracle_gates = world == 1 and not args.no_cpu_baseline and full_legs
    keep_for_gates = {}

    def run_extras():
        if full_legs:
            if args.mode != "cfg4":
                for b in (d_db, d_img, d_pairs, d_cnt):
                    b.free()
                n4 = 10_000_000
                r4 = allpairs_workload(n4, 4, steps=1, warmup=0)
                for b in r4["bufs"]:
                    b.free()
                if want_oracle_gates:
                    keep_for_gates["cfg4"] = (r4["db"], r4["merged"])
                extras["cfg4"] = {"workload": "BASELINE configs[3]: one all-pairs pass over 10M synthetic hashes (4.9999995e13 comparisons), "
                                    f"sharded tile-cyclically over {world} GPU(s), candidates all-gathered ({exchange_kind})",
                        "value": sig(n4 * (n4 - 1) / 2 / r4["elapsed"], 5), "unit": "comparisons/s", "n_gpus": world,
                        "seconds": round(r4["elapsed"], 4), "pairs_found": int(len(r4["merged"])),
                        "per_rank": r4["per_rank"],
                        "roofline": (lambda kms: {"bound": "mfma", "kernel": "k_allpairs_mfma (form chosen by the probe; first-stage MFMAs: 256 flop per comparison)",
                                                  "achieved": sig(n4 * (n4 - 1) / 2 / world * 256.0 / (kms * 1e-3) / 1e12), "peak": FP4_PEAK_TFLOPS,
                                                  "unit": "TFLOP/s", "frac": round(n4 * (n4 - 1) / 2 / world * 256.0 / (kms * 1e-3) / 1e12 / FP4_PEAK_TFLOPS, 4),
                                                  "kernel_ms": round(kms, 3), "traffic": None,
                                                  "basis": "one rank's share of the comparisons over the slowest rank's kernel time (HIP events)"})(
                            max(p_["kernel_ms"] for p_ in r4["per_rank"])),
                        "gate": "every planted pair within tolerance reported; every reported pair re-verified on the host"}
                del r4
        if full_legs and (world == 1 or exchange is not None):  # the hash-shard exchange needs RCCL
            # configs[4]: 50k videos x 64 distinct synthetic 64x64 frames, generated in HBM (13.1 GB over all ranks)
            V, F = args.cfg5_videos, 64
            rng = np.random.default_rng(5)
            copy_of = np.full(V, -1, dtype=np.int32)
            m = int(round(V * 0.02))
            dst = rng.choice(np.arange(1, V), size=m, replace=False)
            is_dst = np.zeros(V, dtype=bool)
            is_dst[dst] = True
            copy_of[dst] = rng.choice(np.flatnonzero(~is_dst), size=m)
            d_copy = L.DeviceBuffer.from_array(copy_of)
            v_lo, v_hi = pipeline.video_range_of_rank(V, rank, world)
            d_frames = L.DeviceBuffer(max(1, (v_hi - v_lo) * F * 4096))
            L.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, v_lo, v_hi - v_lo, F, 5, d_copy.ptr))
            raw_off = np.arange(V + 1, dtype=np.int64) * F
            pipeline.dedupe_frames_on_device(d_frames.ptr, raw_off, 64, 64, 1, 50.0, None, rank, world, exchange)  # warm-up
            times, stage5 = [], []
            for _ in range(3):
                barrier()
                t0 = time.perf_counter()
                tm5 = {}
                pairs5, recs5, lib5 = pipeline.dedupe_frames_on_device(d_frames.ptr, raw_off, 64, 64, 1, 50.0, None, rank,
                                                                       world, exchange, keep_library=True, timings=tm5)
                barrier()
                times.append(rdzv.allreduce_max([time.perf_counter() - t0])[0])
                STAGES5 = ("hash_ms", "gather_ms", "compact_ms", "search_ms", "search_local_ms", "search_exchange_ms", "search_fold_ms")
                stage5.append(rdzv.allreduce_max([tm5[k_] for k_ in STAGES5]))
                mine5 = {k_: round(tm5[k_], 3) for k_ in STAGES5}
                kept5, lens5 = lib5.n_frames, lib5.lengths()
                if want_oracle_gates and len(times) == 3:  # (after the last pass's clock has stopped)
                    keep_for_gates["cfg5"] = {"hashes": lib5.hashes(), "offsets": lib5.offsets(), "recs": recs5, "V": V, "F": F,
                                              "d_frames": d_frames, "video": lib5.d_video.to_array(np.int32, lib5.n_frames)}
                lib5.free()
            fv5 = C.c_int(0)
            L.check(lib.hvd_debug_get(b"mfma_auto_form", C.byref(fv5)))
            probe5 = {}
            for key_ in ("vmatch_bit_order_used", "mfma_auto_half", "mfma_probe_survivors", "mfma_probe_survivors_hi", "mfma_probe_survivors_mix"):
                pv_ = C.c_int(0)
                L.check(lib.hvd_debug_get(key_.encode(), C.byref(pv_)))
                probe5[key_] = pv_.value
            if "cfg5" not in keep_for_gates:
                d_frames.free()
            d_copy.free()
            planted5 = {(int(min(s, d)), int(max(s, d))) for d, s in enumerate(copy_of) if s >= 0}
            found5 = {tuple(p) for p in pairs5.tolist()}
            chk = rdzv.allgather(np.uint64(np.bitwise_xor.reduce(
                recs5.view(np.uint32).astype(np.uint64) * np.arange(1, recs5.size * 4 + 1, dtype=np.uint64)) if recs5.size else 0
            ).tobytes())
            assert len(set(chk)) == 1, "ranks disagree on the config-5 records"
            t5, t5_sd = mean_sd(times)
            fcmp5 = float((lens5.sum() ** 2 - (lens5 ** 2).sum()) / 2)  # frame comparisons between different videos
            hash5_ms, _ = mean_sd([x[0] for x in stage5])
            search5_ms, search5_sd = mean_sd([x[3] for x in stage5])
            stages5 = {k_: round(mean_sd([x[i_] for x in stage5])[0], 3) for i_, k_ in enumerate(STAGES5)}
            per_rank5 = [json.loads(p_) for p_ in rdzv.allgather(json.dumps({"rank": rank, "last_pass": mine5}).encode())]
            # the search's kernel walks every tile of the upper triangle of kept x kept frames (pairs inside one video are
            # computed and then dropped): 2 MFMAs of 2*32*32*64 flop per 1024 comparisons in the first stage; the forms that
            # settle survivors on the matrix pipe execute more (PMC: profiles/r04_pmc_k2_*, r05_pmc_cfg5.txt), the pair-queue form does not
            exec_cmp5 = float(kept5) * (float(kept5) - 1.0) / 2.0 / world
            flop5 = exec_cmp5 / 1024.0 * 2.0 * 131072.0
            search5 = {"ms": round(search5_ms, 3), "ms_sd": round(search5_sd, 3), "form": int(fv5.value),
                       "form_name": {9: "fetch", 12: "register cascade", 18: "pair queue (panel marks)"}.get(int(fv5.value), "?"),
                       "first_stage": {"bit_order_chosen_from_the_library": bool(probe5["vmatch_bit_order_used"]),
                                       "selection": {0: "bits 0..127", 1: "bits 128..255", 2: "bits 0..63 + 192..255"}.get(probe5["mfma_auto_half"], "?")
                                                    + (" of the rewritten hashes" if probe5["vmatch_bit_order_used"] else ""),
                                       "probe_survivors_of_16.7M_sampled_pairs": {"bits 0..127": probe5["mfma_probe_survivors"],
                                                                                  "bits 128..255": probe5["mfma_probe_survivors_hi"],
                                                                                  "bits 0..63 + 192..255": probe5["mfma_probe_survivors_mix"]}},
                       "frame_comparisons_per_s": sig(fcmp5 / (search5_ms * 1e-3)),
                       "executed_comparisons_per_s": sig(exec_cmp5 * world / (search5_ms * 1e-3)),
                       "note": "HIP-event time of the whole hvd_dev_vpdq_match_videos call on the library stream (packed hashes, "
                               "probe, all-pairs pass in video mode, key reduction, record emit; max over ranks)",
                       "roofline": {"bound": "mfma", "kernel": f"k_allpairs_mfma (video mode, form {int(fv5.value)} chosen by the probe)",
                                    "achieved": sig(flop5 / (search5_ms * 1e-3) / 1e12), "peak": FP4_PEAK_TFLOPS, "unit": "TFLOP/s",
                                    "frac": round(flop5 / (search5_ms * 1e-3) / 1e12 / FP4_PEAK_TFLOPS, 4),
                                    "flop_per_launch": flop5,
                                    "basis": "first-stage MFMAs only (2 per 1024 executed comparisons, per rank) over the time of the "
                                             "whole call; counters: profiles/r05_pmc_cfg5.txt (r04_pmc_k2_structured18.txt: stall breakdown)",
                                    "traffic": load_traffic(f"config5_search_v{V}x{F}_w{world}"),
                                    "traffic_source": TRAFFIC_SOURCE}}
            extras["cfg5"] = {"workload": f"BASELINE configs[4]: {V} synthetic videos x {F} distinct 64x64 frames generated in HBM -> PDQ hash -> "
                                "quality filter + CSR on the GPU -> FP4 image -> all video pairs with the vPDQ counters reduced on "
                                f"the GPU -> pair predicate (threshold 50); {world} GPU(s): frames hashed in disjoint video ranges, "
                                f"hash shards all-gathered, search tile-cyclic, key sets all-gathered ({exchange_kind})",
                    "seconds": round(t5, 4), "seconds_sd": round(t5_sd, 4), "n_gpus": world,
                    "frames": V * F, "frames_kept": int(kept5), "videos_per_s": sig(V / t5), "frames_per_s_end_to_end": sig(V * F / t5),
                    "frame_comparisons": fcmp5, "frame_comparisons_per_s_end_to_end": sig(fcmp5 / t5),
                    "hash_ms": round(hash5_ms, 3), "search": search5,
                    "stages_ms": {**stages5,
                                  "what": "max over ranks, mean of 3 passes. hash / search: HIP events on the library stream; gather "
                                          "(all-gather of the hash shards + squeeze), compact (quality filter + CSR), search_local "
                                          "(packed hashes, probe, all-pairs pass, key set), search_exchange (agreement words, key-list "
                                          "all-gather, merged set), search_fold (keys -> pair map): host clock around synchronous steps; "
                                          "the rest of `seconds` is allocation, record read-back and Python"},
                    "per_rank": per_rank5,
                    "video_records": int(len(recs5)), "duplicate_pairs": int(len(pairs5)),
                    "planted_copies": len(planted5), "planted_recall": round(len(planted5 & found5) / max(1, len(planted5)), 4),
                    "gate": "identical record checksum on every rank; at N=1 the cpu_baseline leg puts the oracle behind the WHOLE "
                            "config (full_size_oracle_check: every frame's hash, every record); tests/test_gpu_round5.py does the same"}

    extras_note = None
    if world == 1:
        run_extras()
    elif full_legs:
        import threading

        box = {}

        def guarded():
            try:
                if inproc is not None:
                    L.set_context(rank)  # (the library's current context is per THREAD: this one starts on context 0)
                run_extras()
            except BaseException as exc:  # noqa: BLE001 - reported in the JSON line
                box["err"] = repr(exc)

        th = threading.Thread(target=guarded, daemon=True)
        th.start()
        th.join(float(os.environ.get("HVD_BENCH_EXTRAS_TIMEOUT", "600")))
        if th.is_alive():
            extras_note = "config4/config5 legs did not finish within the deadline (a rank is stuck in an exchange step)"
        elif "err" in box:
            extras_note = "config4/config5 legs failed: " + box["err"]
        if extras_note:
            print(f"[bench] rank {rank}: {extras_note}", file=sys.stderr)
            hard_exit = True
    cfg4, cfg5 = extras.get("cfg4"), extras.get("cfg5")
    cfg5_note = None
    if cfg5 is None and full_legs and not extras_note and world > 1 and exchange is None:
        # (said out loud: a line without config5 must be readable as "skipped, and why", not as a failure)
        cfg5_note = ("config5 leg skipped: its hash-shard and key-list exchanges run inside the library over RCCL, and this run "
                     f"exchanges over {exchange_kind}")

    if rank != 0:
        if extras_note:  # do not enter another collective: rank 0 prints what it has
            if inproc is not None:
                return  # (a thread of the single process: rank 0's thread prints and ends the process)
            os._exit(0)
        if exchange is not None:
            exchange.close()
        rdzv.barrier()
        rdzv.close()
        if hard_exit:
            os._exit(0)
        return

    # kernel-level roofline (one rank's share of the comparisons per launch)
    cmp_per_launch = total_cmp / world
    achieved = cmp_per_launch * BYTES_PER_COMPARISON / (kernel_avg_ms * 1e-3) / 1e9
    traffic = load_traffic(f"allpairs_n{n}_v{variant}_w{world}")
    if traffic is None and variant == 13:
        traffic = load_traffic(f"allpairs_n{n}_v9_w{world}")
    hbm_equiv = {"achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": round(achieved / HBM_PEAK_GBS, 3),
                 "note": "SURVEY.md 8d accounting: 64 B per comparison with no operand reuse credited; frac > 1 "
                         "because tiles re-use operands from registers/LDS"}
    if variant >= 8:
        # executed matrix work: 2 (128-bit first stage) or 4 MFMAs of 2*32*32*64 flop per 1024 comparisons
        flop_per_cmp = 256.0 if form in (9, 12, 18) else 512.0
        tfl = cmp_per_launch * flop_per_cmp / (kernel_avg_ms * 1e-3) / 1e12
        roofline = {"bound": "mfma", "kernel": f"k_allpairs_mfma(variant={variant}" + (f" -> form {form} chosen by the probe)" if variant == 13 else ")"),
                    "achieved": round(tfl, 1),
                    "peak": FP4_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tfl / FP4_PEAK_TFLOPS, 3),
                    "traffic": traffic, "traffic_source": TRAFFIC_SOURCE if traffic is not None else None,
                    "kernel_ms": round(kernel_avg_ms, 3), "kernel_ms_sd_rank0": round(k_sd, 3),
                    "instr": "v_mfma_f32_32x32x64_f8f6f4 cbsz:4 blgp:4 on the +-1 FP4 image of the hashes",
                    "flop_per_comparison_executed": flop_per_cmp, "hbm_equivalent": hbm_equiv,
                    "note": "kernel_ms covers everything between the HIP events of one pass: probe + form selection + the "
                            "all-pairs kernel; `achieved` counts only the first-stage MFMAs every comparison executes"}
        # the clock the timed passes actually ran at (in-kernel s_memtime / s_memrealtime, slowest rank) and the roofline against
        # the peak AT THAT CLOCK: tells a slow box (power-limited clock) from a slow kernel
        slow = max(head["per_rank"], key=lambda p_: p_["kernel_ms"])
        if slow.get("effective_mhz"):
            roofline["effective_mhz"] = slow["effective_mhz"]
            roofline["clock_samples"] = slow["clock_samples"]
            roofline["peak_at_clock"] = round(FP4_PEAK_TFLOPS * slow["effective_mhz"] / MAX_SCLK_MHZ, 1)
            roofline["frac_at_clock"] = round(tfl / (FP4_PEAK_TFLOPS * slow["effective_mhz"] / MAX_SCLK_MHZ), 3)
            roofline["clock_note"] = (f"peak quoted at {MAX_SCLK_MHZ:.0f} MHz; effective_mhz = shader cycles / constant-rate ticks of one "
                                      "workgroup in eight of the timed passes (k_allpairs_mfma); frac_at_clock = achieved / (peak x "
                                      "effective_mhz / 2400): pipe utilisation at the clock the power limit allowed")
    else:
        roofline = {"bound": "hbm", "kernel": f"k_allpairs(variant={variant})", "traffic": traffic,
                    "traffic_source": TRAFFIC_SOURCE if traffic is not None else None,
                    "kernel_ms": round(kernel_avg_ms, 3), **hbm_equiv,
                    "note": hbm_equiv["note"] + "; binding unit: integer VALU (v_bcnt_u32_b32 issues at half rate, "
                                                "profiles/r01_ubench_valu.txt)"}

    frames_out = None
    if args.full:
        fps = world * args.frames / (k1_ms * 1e-3)
        frames_out = {
            "workload": f"{args.frames} pre-decoded synthetic 64x64 gray frames per GPU -> PDQ hash + quality "
                        "(BASELINE configs[1]; frames are independent, ranks hash disjoint batches, no collective)",
            "value": sig(fps), "unit": "frames/s", "kernel_ms": round(k1_ms, 4), "kernel_ms_sd": round(k1_sd, 4), "dtype": "f32",
            "warmup_launches": K1_WARM, "timed_launches": 50,
            "value_idle_chip": sig(world * args.frames / (k1_idle_ms * 1e-3)), "kernel_ms_idle_chip": round(k1_idle_ms, 4),
            "order_note": "`value` is measured right after the headline's matrix-core passes (clocks still power-limited), "
                          "`value_idle_chip` before them",
            "n_gpus": world, "wall_value": sig(world * args.frames * 50 / k1_wall),
            "roofline": k1_roofline(fps / world, load_traffic(f"pdq_hash64_n{args.frames}")),
        }

    out = {
        "metric": "hash-pair comparisons/sec", "value": sig(value, 5), "unit": "comparisons/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "fp4(e2m1, +-1 image of the hash bits) x fp4 -> f32, exact" if variant >= 8 else "u32", "data": "synthetic",
        "config": {"workload": f"all-pairs 256-bit Hamming (tolerance 31) over {n} synthetic hashes with planted "
                               f"near-duplicates, {total_cmp:.6g} comparisons per step ({wl})",
                   "n_hashes": n, "max_dist": 31, "kernel_variant": variant, "mode": args.mode,
                   "parallelism": f"tile-cyclic x{world}, DB replicated, exchange={exchange_kind}",
                   "exchange": exchange_kind, "rccl_ranks": world if exchange_kind == "rccl" else 0,
                   "launch": "single process: the library's device group (hvd_init_devices), one thread per GPU" if inproc is not None
                             else "one process per GPU",
                   "pairs_found": int(len(merged))},
        "roofline": roofline,
        "per_rank": head["per_rank"],
        # which block is the scaling curve: the top-level `value` at every N
        "scale_metric": {
            "weak": f"`value`: all-pairs comparisons/s over n = {args.hashes}*sqrt(N) hashes (comparisons per GPU fixed at "
                    f"{args.hashes * (args.hashes - 1) // 2:.4g}; BASELINE configs[2] at N=1); with --full, `config4.value` is the "
                    "strong-scaling companion (BASELINE configs[3], 10M hashes, fixed total work) measured in the same run",
            "strong": "`value`: all-pairs comparisons/s over BASELINE configs[2] (fixed total work) at every N",
            "cfg4": "`value`: all-pairs comparisons/s over BASELINE configs[3] (10M hashes, fixed total work) at every N",
        }[args.mode],
    }
    if world > 1:
        # what this line is to be held against: the step time predicted from the N = 1 measurements and the
        # exact tile partition (hvd_amd.multigpu.SCALING_MODEL / predict_step; table in DESIGN.md section 5)
        try:
            pred = M.predict_step(n, world)
            pred1 = M.predict_step(args.hashes, 1)
            pred["efficiency"] = round(pred["comparisons_per_s"] / (world * pred1["comparisons_per_s"]), 3)
            pred["basis"] = ("N = 1 measurements of round 6 (kernel 3.62 ms per 1e11 comparisons, fixed per-step pieces) + the exact "
                             "work share of the slowest rank; not fitted to any multi-GPU run")
            pred["measured_over_predicted"] = round(ms_per_step / pred["ms_per_step"], 3)
            out["predicted"] = pred
            if strong:
                ps = M.predict_step(args.hashes, world)
                ps["efficiency"] = round(ps["comparisons_per_s"] / (world * pred1["comparisons_per_s"]), 3)
                ps["measured_over_predicted"] = round(strong["ms_per_step"] / ps["ms_per_step"], 3)
                strong["predicted"] = ps
        except Exception as exc:  # noqa: BLE001 - a diagnostics block must not be able to take the measurement with it
            out["predicted"] = {"error": repr(exc)}
    if strong:
        out["strong"] = strong
    if cfg4:
        out["config4"] = cfg4
    if cfg5:
        out["config5"] = cfg5
    if extras_note:
        out["extras_note"] = extras_note
    if cfg5_note:
        out["config5_note"] = cfg5_note
    if dumped:
        out["dump_outputs"] = dumped

    cpu = None
    if world == 1 and full_legs:
        extra = {}
        # chip-filling batch of the 64x64 hash kernel (10k frames occupy a fraction of the 256 CUs' wave slots)
        _, dh2, dq2, kl, _ = time_k1(400_000, 10)
        dh2.free()
        dq2.free()
        m400, s400 = mean_sd(kl)
        frames_out["batch_400k"] = {"workload": "400 000 frames in one launch: the 10 000 distinct frames of configs[1] x 40 on the device",
                                    "value": sig(400_000 / (m400 * 1e-3)), "unit": "frames/s", "kernel_ms": round(m400, 3),
                                    "kernel_ms_sd": round(s400, 3),
                                    "roofline": k1_roofline(400_000 / (m400 * 1e-3), load_traffic("pdq_hash64_n400000"))}

        # the headline DB again for the side-by-side legs
        d_db = L.DeviceBuffer.from_array(db)
        img_bytes = C.c_size_t(0)
        L.check(lib.hvd_fp4_image_bytes(n, C.byref(img_bytes)))
        d_img = L.DeviceBuffer(img_bytes.value)
        cap = 1 << 23
        d_pairs = L.DeviceBuffer(16 * cap)
        d_cnt = L.DeviceBuffer(8)
        L.check(lib.hvd_dev_expand_fp4(d_db.ptr, n, d_img.ptr))

        def time_variant(v, reps=5, d_db_=None, d_img_=None):
            ks = []
            for r in range(reps + 1):
                d_cnt.zero()
                L.check(lib.hvd_timer_start())
                M.launch_allpairs(lib, (d_db_ or d_db).ptr, (d_img_ or d_img).ptr, n, None, 31, 0, 1, d_pairs.ptr, cap,
                                  d_cnt.ptr, v)
                ms = C.c_float(0)
                L.check(lib.hvd_timer_stop(C.byref(ms)))
                if r:
                    ks.append(ms.value)
            return mean_sd(ks) + (int(d_cnt.to_array(np.uint64, 1)[0]),)

        # every exact form next to the default, for transparency (same DB, same launch shape)
        for v, name in ((0, "popcount_full_16op"), (1, "popcount_prefilter128"), (8, "mfma_fp4_full_256"),
                        (9, "mfma_fp4_stage128_fetch"), (12, "mfma_fp4_stage128_registers"),
                        (18, "mfma_fp4_stage128_panel_mark_queue")):
            mu, sd, _ = time_variant(v, reps=3)
            extra[name] = {"kernel_ms": round(mu, 3), "kernel_ms_sd": round(sd, 3), "comparisons_per_s": sig(total_cmp / (mu * 1e-3))}
        out["kernel_variants"] = extra

        # CLUSTERED hash DBs: the regime of real frame hashes (static scenes, re-encodes), where many panels contain a
        # hit and take the kernel's slow path; the uniform DB above never does.
        clustered = {}
        for name, (ncl, csz) in (("1e4_clusters_of_10", (10_000, 10)), ("1e3_clusters_of_100", (1_000, 100))):
            dbc, members = synth.hash_db_clustered(n, ncl, csz, seed=8)
            d_dbc = L.DeviceBuffer.from_array(dbc)
            d_imgc = L.DeviceBuffer(img_bytes.value)
            L.check(lib.hvd_dev_expand_fp4(d_dbc.ptr, n, d_imgc.ptr))
            mu, sd, cnt = time_variant(variant, reps=5, d_db_=d_dbc, d_img_=d_imgc)
            want_pairs = ncl * csz * (csz - 1) // 2
            assert cnt == want_pairs, (cnt, want_pairs)  # every in-cluster pair, nothing else
            got = d_pairs.to_array(L.PAIR_DTYPE, cnt)[:: max(1, cnt // 20000)]
            dd = np.unpackbits(dbc[got["i"]] ^ dbc[got["j"]], axis=1).sum(1)
            assert np.array_equal(dd, got["dist"]) and (got["i"] < got["j"]).all()
            p_pair = (csz - 1) / n
            clustered[name] = {"kernel_ms": round(mu, 3), "kernel_ms_sd": round(sd, 3),
                               "comparisons_per_s": sig(total_cmp / (mu * 1e-3)), "pairs": cnt,
                               "slow_path_share_of_panels": round(1.0 - math.exp(-8192 * p_pair), 3),
                               "form": None,
                               "vs_uniform": round(k_mean / mu, 3)}
            if variant == 13:
                fv = C.c_int(0)
                L.check(lib.hvd_debug_get(b"mfma_auto_form", C.byref(fv)))
                clustered[name]["form"] = fv.value
            d_dbc.free()
            d_imgc.free()
            del dbc
        out["clustered_db"] = {"workload": f"{n} hashes, clusters of near-identical hashes (<= 16 bits apart) scattered uniformly "
                                           "over the DB; all in-cluster pairs must come back (count and sampled distances "
                                           "verified); slow_path_share = expected share of (wave, 32-candidate panel) steps "
                                           "that contain a hit", **clustered}

        # the reference's real frame geometry: 512x512 packed RGB24 (vpdqpy/vpdqpy.py:90-95)
        n_rgb = 6144  # two full rounds of the 3072 resident waves of k_down512w (4.8 GB of frames)
        rgb = synth.frames_rgb(16, seed=6)
        sb = C.c_size_t(0)
        L.check(lib.hvd_pdq_scratch_bytes(n_rgb, 512, 512, 3, C.byref(sb)))
        d_rf = L.DeviceBuffer(n_rgb * 786432)
        for rep in range(n_rgb // 16):  # the 16 distinct frames, replicated on the device
            L.check(lib.hvd_memcpy_h2d(C.c_void_p(d_rf.ptr + rep * rgb.nbytes), rgb.ctypes.data, rgb.nbytes))
        d_rs = L.DeviceBuffer(sb.value)
        d_rh = L.DeviceBuffer(32 * n_rgb)
        d_rq = L.DeviceBuffer(4 * n_rgb)
        rl = []
        RGB_WARM = 30  # the chip comes out of a host-side pause: launch times fall for ~20 launches before they settle
        for r in range(RGB_WARM + 10):  # mean of 10 after the warm-up (same statistic as every other leg)
            L.check(lib.hvd_timer_start())
            L.check(lib.hvd_dev_pdq_hash_frames(d_rf.ptr, n_rgb, 512, 512, 3, d_rs.ptr, d_rh.ptr, d_rq.ptr))
            ms = C.c_float(0)
            L.check(lib.hvd_timer_stop(C.byref(ms)))
            if r >= RGB_WARM:
                rl.append(ms.value)
        rgb_ms, rgb_sd = mean_sd(rl)
        rgb_fps = n_rgb / (rgb_ms * 1e-3)
        frames_out["rgb24_512x512"] = {
            "warmup_launches": RGB_WARM,
            "workload": f"{n_rgb} pre-decoded synthetic 512x512 RGB24 frames (16 distinct frames x {n_rgb // 16} on the device; "
                        "the reference's hash_frame input): luma + 2x Jarosz + decimate (k_down512w, one wave per frame) + "
                        "k_pdq_hash64",
            "value": sig(rgb_fps), "unit": "frames/s", "ms": round(rgb_ms, 3), "ms_sd": round(rgb_sd, 3),
            "roofline": {"bound": "hbm", "kernel": "k_down512w", "achieved": round(rgb_fps * BYTES_PER_FRAME_RGB512 / 1e9, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(rgb_fps * BYTES_PER_FRAME_RGB512 / 1e9 / HBM_PEAK_GBS, 3),
                         "traffic": load_traffic(f"down512w_rgb_n{n_rgb}"), "traffic_source": TRAFFIC_SOURCE,
                         "note": "algorithmic bytes = 786432 in + 36 out per frame; `traffic` = PMC bytes per launch "
                                 "(FETCH_SIZE x2 + WRITE_SIZE, profiles/)"}}

        out["videohasher_stream"] = videohasher_stream_leg(lib, L, synth, hvd_amd.vpdq)

        # sustained: the headline pass back to back with no host synchronisation in between (power/thermal steady state)
        if args.sustain_seconds > 0:
            reps = max(10, int(args.sustain_seconds / (k_mean * 1e-3)))
            d_cnt.zero()
            if variant >= 8:
                L.check(lib.hvd_debug_set(b"mfma_clock_reset", 1))
            with PowerSampler(my_pci) as ps:  # power / clock read-outs every 50 ms while the passes run (host thread, sysfs)
                L.check(lib.hvd_timer_start())
                for _ in range(reps):
                    if variant >= 8:
                        L.check(lib.hvd_dev_expand_fp4(d_db.ptr, n, d_img.ptr))
                    M.launch_allpairs(lib, d_db.ptr, d_img.ptr, n, None, 31, 0, 1, d_pairs.ptr, cap, d_cnt.ptr, variant)
                ms = C.c_float(0)
                L.check(lib.hvd_timer_stop(C.byref(ms)))
            assert int(d_cnt.to_array(np.uint64, 1)[0]) == reps * len(merged)
            s_mhz, s_n = pass_clock_mhz(lib, L) if variant >= 8 else (None, 0)
            out["sustained"] = {"what": f"{reps} passes (FP4 image + all-pairs) enqueued back to back, one synchronisation at the end",
                                "seconds": round(ms.value / 1e3, 2), "ms_per_pass": round(ms.value / reps, 3),
                                "comparisons_per_s": sig(total_cmp / (ms.value / reps * 1e-3)),
                                "effective_mhz": round(s_mhz, 1) if s_mhz else None, "clock_samples": s_n,
                                "sysfs_during": ps.summary()}
        for b in (d_db, d_img, d_pairs, d_cnt):
            b.free()

        if not args.no_cpu_baseline:
            from oracle import oracle as O  # cpu_baseline leg only

            cores = host_threads()
            # The baseline builds: the oracle recompiled ON this box with -O3 -march=native, and the portable
            # -O2 -mpopcnt library that travels with the repo. Both select the AVX-512 VPOPCNTDQ block scan at run time
            # where CPUID offers it. `value` is the FASTER of the two (the baseline must be the best CPU
            # number this run measured), each timed on the same bounded sample: calibrate, then ~cpu-seconds/2 of work each.
            def cpu_pass(n_, threads, native):
                t_ = time.perf_counter()
                c_ = O.allpairs_count(db[:n_], 31, num_threads=threads, native=native)
                dt_ = time.perf_counter() - t_
                return (n_ * (n_ - 1) / 2) / dt_, dt_, c_

            n0 = min(n, 150_000)  # big enough that thread start-up does not dominate on many-core hosts
            cal = {}
            for native in (True, False):
                cpu_pass(n0, cores, native)  # warm: build, page in, spawn once
                cal[native] = cpu_pass(n0, cores, native)[0]
            ns = int(min(n, max(n0, math.sqrt(2 * max(cal.values()) * args.cpu_seconds / 2))))
            if n * (n - 1) / 2 / max(cal.values()) <= max(12.0, args.cpu_seconds / 2):
                ns = n  # the whole DB is affordable (<= 12 s per build): the sample doubles as the full-size parity gate
            runs = {native: cpu_pass(ns, cores, native) for native in (True, False)}
            best_native = runs[True][0] >= runs[False][0]
            cpu_cmp, dt, cpu_count = runs[best_native]
            assert runs[True][2] == runs[False][2], "the two oracle builds disagree on the pair count"
            # Full-size differential gate: when the sample IS the whole DB, the oracle's pair count must
            # equal the GPU's. Together with the gate above (every GPU pair re-verified on the host with its distance, no
            # pair reported twice) equal counts mean equal SETS: the GPU's pairs are all true, and none is missing.
            full_size_check = None
            if ns == n:
                assert cpu_count == len(merged), f"oracle counts {cpu_count} pairs over the full DB, the GPU reported {len(merged)}"
                full_size_check = True
            n1 = min(n, 60_000)  # single-thread figure on a smaller prefix (~1-2 s)
            cpu_cmp_1t = cpu_pass(n1, 1, best_native)[0]
            native_flags, portable_flags = O.native_lib().flags, O.PORTABLE_FLAGS
            cpu_flags = {"value_build": native_flags if best_native else portable_flags,
                         "avx512_vpopcntdq": O.uses_avx512(best_native),
                         "native_build": native_flags, "native_value": sig(runs[True][0]),
                         "native_avx512_vpopcntdq": O.uses_avx512(True),
                         "portable_build": portable_flags, "portable_value": sig(runs[False][0]),
                         "portable_avx512_vpopcntdq": O.uses_avx512(False),
                         "both_on_sample": f"first {ns} hashes, {cores} threads"}
            # K1 on the CPU: >= 1.5 s of work in calls of 16 x the 10k frames each (one call = 160k frames, so the thread
            # start-up of a call is noise); the first call is a warm-up and doubles as the parity check of the GPU hashes
            ho, qo = O.hash_frames(fr, num_threads=cores)
            fr_rep = np.ascontiguousarray(np.tile(fr, (16, 1, 1)))
            O.hash_frames(fr_rep[: fr.shape[0] * 2], num_threads=cores)
            dtf, nf_cpu = 0.0, 0
            while dtf < 1.5:
                t = time.perf_counter()
                O.hash_frames(fr_rep, num_threads=cores)
                dtf += time.perf_counter() - t
                nf_cpu += fr_rep.shape[0]
            del fr_rep
            hg = d_h.to_array(np.uint8, 32 * args.frames).reshape(-1, 32)
            qg = d_q.to_array(np.int32, args.frames)
            assert np.array_equal(hg, ho) and np.array_equal(qg, qo), "GPU frame hashes differ from the oracle"
            rgb_rep = np.concatenate([rgb] * 16)  # 256 frames per call, repeated to >= 1 s
            hro, qro = O.hash_frames(rgb_rep, num_threads=cores)
            dtr, nr_cpu = 0.0, 0
            while dtr < 1.0:
                t = time.perf_counter()
                O.hash_frames(rgb_rep, num_threads=cores)
                dtr += time.perf_counter() - t
                nr_cpu += 256
            hr = d_rh.to_array(np.uint8, 32 * n_rgb).reshape(-1, 32)
            qr = d_rq.to_array(np.int32, n_rgb)
            assert (np.array_equal(hr, np.tile(hro[:16], (n_rgb // 16, 1))) and
                    np.array_equal(qr, np.tile(qro[:16], n_rgb // 16))), "GPU rgb512 hashes differ from the oracle"
            frames_out["rgb24_512x512"]["cpu_frames_per_s"] = sig(nr_cpu / dtr)
            frames_out["rgb24_512x512"]["cpu_sample"] = f"{nr_cpu} frames, {cores} threads, {dtr:.2f} s"
            # K3: 2000 videos x 64 frame hashes, every video pair; host buffers in, records out
            vfr, voff, _ = synth.video_hashes(2000, seed=7, frames_per_video=64, copy_fraction=0.02)
            search.match_videos(vfr[:6400], voff[:101])  # warm
            t = time.perf_counter()
            rec_g = search.match_videos(vfr, voff)
            dt_g = time.perf_counter() - t
            O.match_videos(vfr[:6400], voff[:101], num_threads=cores)  # warm
            t = time.perf_counter()
            rec_c = O.match_videos(vfr, voff, num_threads=cores)
            dt_c = time.perf_counter() - t
            assert np.array_equal(rec_g, rec_c), "GPU video-match records differ from the oracle"
            k3_cmp = 2000 * 1999 // 2 * 4096
            out["video_match"] = {"workload": "2000 synthetic videos x 64 frame hashes, all video pairs (hvd_vpdq_match_videos, "
                                              "host buffers in, video-level records out; counters reduced on the GPU)",
                                  "value": sig(k3_cmp / dt_g), "unit": "frame comparisons/s", "ms": round(dt_g * 1e3, 2),
                                  "records": int(len(rec_g)), "cpu_value": sig(k3_cmp / dt_c), "cpu_threads": cores,
                                  "note": "small problem: transfer + launch overheads dominate the GPU figure; config5 above is "
                                          "the same path at full size"}
            cpu = {"value": sig(cpu_cmp), "unit": "comparisons/s", "cores": cores, "kind": "port", "flags": cpu_flags,
                   "sample": f"oracle (C, pthreads; {cpu_flags['value_build']}; "
                             f"{'AVX-512 VPOPCNTDQ block scan' if cpu_flags['avx512_vpopcntdq'] else 'scalar popcnt loop'}) "
                             f"all-pairs over the first {ns} of the {n} hashes "
                             f"({ns * (ns - 1) // 2:.3g} comparisons, {dt:.1f} s)",
                   "value_1thread": sig(cpu_cmp_1t),
                   "speedup_over_1thread": round(cpu_cmp / cpu_cmp_1t, 1), "os_cpu_count": os.cpu_count(),
                   "frames_per_s": sig(nf_cpu / dtf),
                   "frames_sample": f"oracle PDQ over the same {args.frames} frames x {nf_cpu // args.frames} "
                                    f"({nf_cpu} frames in calls of {16 * args.frames}), {cores} threads, {dtf:.2f} s",
                   "frames_sample_seconds": round(dtf, 2),
                   "full_size_oracle_check": full_size_check,
                   "note": "the reference's real CPU path (hvdaccelerators 0.4.0) is not installable offline; this "
                           "is the oracle port"}

            # ---- full-size oracle gates: the two BASELINE configs no sampled check had behind them ----
            # config4 (10M hashes): the oracle scans EVERY column for the rows of 40+ bands (random, first, last, one per rank
            # straddling a row-block boundary); the GPU list restricted to those rows must be the oracle's, record for record.
            if "cfg4" in keep_for_gates and cfg4 is not None:
                db4, merged4 = keep_for_gates.pop("cfg4")
                n4_ = db4.shape[0]
                bands4 = oracle_check_bands(n4_, M.tile_geometry(n4_, 9)[0], 8, seed=46)
                est = sum((b_ - a_) * (n4_ - (a_ + b_) / 2.0) for a_, b_ in bands4) / cpu_cmp + 2.0
                if est > args.oracle_check_seconds:
                    cfg4["oracle_band_check"] = None
                    cfg4["oracle_band_check_note"] = f"skipped: estimated {est:.0f} s of CPU work > --oracle-check-seconds {args.oracle_check_seconds:.0f}"
                else:
                    t_ = time.perf_counter()
                    want4 = O.allpairs_bands(db4, bands4, 31, num_threads=cores)
                    in_band = np.zeros(n4_, dtype=bool)
                    for a_, b_ in bands4:
                        in_band[a_:b_] = True
                    got4 = merged4[in_band[merged4["i"]]]
                    assert len(got4) == len(want4) and all(np.array_equal(got4[f_], want4[f_]) for f_ in ("i", "j", "dist")), \
                        f"config4: GPU pair list differs from the oracle on the sampled row bands ({len(got4)} vs {len(want4)} records)"
                    cfg4["oracle_band_check"] = True
                    cfg4["oracle_band_check_note"] = (f"{len(bands4)} row bands ({sum(b_ - a_ for a_, b_ in bands4)} rows x every column j > i of the "
                                                      f"{n4_} hashes), {len(want4)} records equal, {time.perf_counter() - t_:.1f} s on {cores} threads")
                del db4, merged4
            # config5 (50k videos x 64 frames): every frame hashed by the oracle -> kept hashes and CSR byte-equal to the device
            # library's; the oracle's scan over all kept x kept frame pairs with the video group filter, folded on the host to
            # video-level counters, equal to the product's hvd_vmatch records.
            if "cfg5" in keep_for_gates and cfg5 is not None:
                k5 = keep_for_gates.pop("cfg5")
                nfr5, kept5_ = k5["V"] * k5["F"], k5["hashes"].shape[0]
                est = nfr5 / (nf_cpu / dtf) + kept5_ * (kept5_ - 1) / 2.0 / cpu_cmp + 3.0
                if est > args.oracle_check_seconds:
                    cfg5["full_size_oracle_check"] = None
                    cfg5["full_size_oracle_check_note"] = f"skipped: estimated {est:.0f} s of CPU work > --oracle-check-seconds {args.oracle_check_seconds:.0f}"
                else:
                    t_ = time.perf_counter()
                    ho5, qo5 = oracle_hash_device_frames(L, O, k5["d_frames"].ptr, nfr5, cores)
                    t_h = time.perf_counter() - t_
                    keep5 = qo5 >= 31
                    off5 = np.zeros(k5["V"] + 1, dtype=np.int64)
                    np.cumsum(keep5.reshape(k5["V"], k5["F"]).sum(1), out=off5[1:])
                    kept_o5 = np.ascontiguousarray(ho5[keep5])
                    assert np.array_equal(k5["offsets"], off5), "config5: per-video CSR of the kept frames differs from the oracle's"
                    assert np.array_equal(k5["hashes"], kept_o5), "config5: kept frame hashes differ from the oracle's"
                    fp5 = O.allpairs(kept_o5, 31, group=k5["video"], cap=1 << 22, num_threads=cores)
                    want5 = fold_frame_pairs(fp5, k5["video"], k5["V"], L.VMATCH_DTYPE)
                    assert np.array_equal(k5["recs"], want5), \
                        f"config5: video records differ from the fold of the oracle's frame pairs ({len(k5['recs'])} vs {len(want5)})"
                    cfg5["full_size_oracle_check"] = True
                    cfg5["full_size_oracle_check_note"] = (f"oracle hashed all {nfr5} frames ({t_h:.1f} s): {kept5_} kept hashes + CSR byte-equal; "
                                                           f"oracle scan of {kept5_ * (kept5_ - 1) / 2.0:.4g} frame pairs with the video filter -> "
                                                           f"{len(fp5)} frame pairs -> {len(want5)} video records equal; "
                                                           f"{time.perf_counter() - t_:.1f} s on {cores} threads")
                    cfg5["cpu_frames_per_s_full_library"] = sig(nfr5 / t_h)
                k5["d_frames"].free()
                del k5

        # the reference-shaped loop -- one Python call per video pair, as db/vptree.py:29-31,737 issues them
        # (tests/benchmarks/test_benchmark_vpdqpy.py:62-73 has the same shape). 64-frame hashes, 1024 calls.
        vf, voff, _ = synth.video_hashes(33, seed=1, frames_per_video=64, copy_fraction=0.1)
        blobs = [vf[voff[v]:voff[v + 1]].tobytes() for v in range(33)]
        hvd_amd.calculate_distance(blobs[0], blobs[1])
        t = time.perf_counter()
        ncall = 0
        for a_ in range(32):
            for b_ in range(32):
                hvd_amd.calculate_distance(blobs[a_], blobs[b_ + 1])
                ncall += 1
        per_call = (time.perf_counter() - t) / ncall
        out["reference_shaped_loop"] = {
            "what": "calculate_distance(a, b) = fix_vpdq_similarity(matchHashBytes(a, b, 31)) on 64-frame video hashes, "
                    "one call per pair from Python (the reference's VP-tree call pattern)",
            "us_per_call": round(per_call * 1e6, 1), "calls": ncall,
            "frame_comparisons_per_s": sig(4096 / per_call, 3),
            "note": "latency-bound by construction (round 5: served by a resident workgroup that polls pinned host memory, no launch "
                    "per call); the batch entry points above replace the loop, not the callee"}

        # the unchanged pipeline's search loop (dedup.py:468-491) against the VpTreeManager-compatible facade: one cached GPU
        # pass, then one lookup + SQL fan-out per file
        import sqlite3

        from hvd_amd import vptree as VT

        nv = 100_000
        vfr2, voff2, _ = synth.video_hashes(nv, seed=11, frames_per_video=64, copy_fraction=0.05)
        conn = sqlite3.connect(":memory:")
        conn.execute("CREATE TABLE files ( hash_id INTEGER PRIMARY KEY, file_hash BLOB_BYTES UNIQUE )")
        conn.execute("CREATE TABLE shape_perceptual_hashes ( phash_id INTEGER PRIMARY KEY, phash BLOB_BYTES UNIQUE )")
        conn.execute("CREATE TABLE shape_perceptual_hash_map ( phash_id INTEGER, hash_id INTEGER, PRIMARY KEY ( phash_id, hash_id ) )")
        conn.execute("CREATE TABLE shape_search_cache ( hash_id INTEGER PRIMARY KEY, searched_distance INTEGER )")
        conn.executemany("INSERT INTO files VALUES (?, ?)", ((v + 1, f"{v:064x}") for v in range(nv)))
        conn.executemany("INSERT INTO shape_perceptual_hashes VALUES (?, ?)",
                         ((v + 1, vfr2[voff2[v]:voff2[v + 1]].tobytes()) for v in range(nv)))
        conn.executemany("INSERT INTO shape_perceptual_hash_map VALUES (?, ?)", ((v + 1, v + 1) for v in range(nv)))
        conn.executemany("INSERT INTO shape_search_cache VALUES (?, NULL)", ((v + 1,) for v in range(nv)))
        del vfr2
        tree = VT.VpTreeManager(conn)
        t = time.perf_counter()
        tree.search_file(1, 51)  # first search: library read + upload + the one GPU pass + the fold into neighbour lists
        t_first = time.perf_counter() - t
        t = time.perf_counter()
        found = 0
        for v in range(nv):  # dedup.py:468-491: search, then record the searched distance (which moves the change counter)
            found += len(tree.search_file(v + 1, 51)) - 1
            conn.execute("UPDATE shape_search_cache SET searched_distance = ? WHERE hash_id = ?;", (51, v + 1))
        per_file = (time.perf_counter() - t) / nv
        t = time.perf_counter()
        for v in range(nv):
            conn.execute("UPDATE shape_search_cache SET searched_distance = ? WHERE hash_id = ?;", (51, v + 1))
        per_update = (time.perf_counter() - t) / nv
        out["vptree_facade_loop"] = {
            "what": f"the reference's search loop (dedup.py:468-491) over an SQLite library of {nv} files (64-frame hashes): "
                    "VpTreeManager.search_file(hash_id, 51) + the shape_search_cache UPDATE per file; the facade answers from "
                    "one cached brute-force GPU pass and an in-memory copy of the phash<->file map",
            "files": nv, "first_search_s": round(t_first, 3), "us_per_file": round((per_file - per_update) * 1e6, 2),
            "us_per_file_with_the_loops_own_update": round(per_file * 1e6, 2), "similar_found": found,
            "frame_comparisons_replaced_per_file": nv * 4096,
            "note": "the reference's tree costs O(visited nodes) matchHashBytes calls per file (18 us each through this "
                    "package's per-pair entry: reference_shaped_loop)"}
        conn.close()

    if frames_out:
        out["frames_hashed"] = frames_out
    for pr in head["per_rank"]:  # clock / power of the timed region, per device
        rk = next((r_ for r_ in runtime.get("ranks", []) if r_.get("rank") == pr["rank"]), None)
        dev = next((d_ for d_ in runtime.get("devices", []) if rk and d_.get("pci") == rk.get("pci")), None)
        tel = {"rank": pr["rank"], "effective_mhz_timed_passes": pr.get("effective_mhz"), "clock_samples": pr.get("clock_samples"),
               "sysfs_before_timed_region": pr.get("sysfs_before"), "sysfs_after_timed_region": pr.get("sysfs_after")}
        if dev is not None:
            dev.setdefault("telemetry", []).append(tel)
        else:
            runtime.setdefault("telemetry_unmatched", []).append(tel)
    out["runtime"] = runtime
    out["policies"] = policies
    out["traffic_provenance"] = traffic_provenance()
    if cpu:
        out["cpu_baseline"] = cpu
        out["full_size_oracle_check"] = cpu["full_size_oracle_check"]
    real_stdout.write(json.dumps(out) + "\n")
    real_stdout.flush()
    if extras_note:
        os._exit(0)
    if exchange is not None:
        exchange.close()
    rdzv.barrier()
    rdzv.close()
    if hard_exit:
        os._exit(0)


if __name__ == "__main__":
    main()
