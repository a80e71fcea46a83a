"""Batch pipeline over a whole library: hash every video's frames in one pass over HBM, then
search all video pairs (BASELINE config 5 shape). The reference does this one video at a time
(`dedup.py:346-352`) and one tree probe per video (`dedup.py:468-475`); a GPU wants the batch.

Two forms:

* host arrays in, Python objects out (`hash_videos`, `dedupe_videos`) -- convenience, mirrors the
  per-video API;
* **device-resident** (`DeviceLibrary`, `dedupe_frames_on_device`): frames already in HBM are hashed,
  the quality filter (`VideoHasher.finish`, vpdqpy/vpdqpy.py:119: quality >= 31 kept,
  db/DedupeDB.py:550-553) runs as a stream compaction on the GPU together with the per-video CSR
  offsets, the kept hashes are rewritten as their FP4 image and searched, and the video-level
  vPDQ counters are reduced on the GPU. Nothing but `hvd_vmatch` records and the V+1 offsets
  crosses PCIe. With one process per GPU the frames are hashed in disjoint video ranges and the
  hash shards are all-gathered over RCCL before the sharded search.
"""

from __future__ import annotations

import ctypes as C
import threading
import time
from collections import namedtuple

import numpy as np

from . import _lib, search, vpdq
from ._lib import GROUP_DTYPE, VMATCH_DTYPE, DeviceBuffer


def hash_videos(videos, autocrop=False) -> list[vpdq.VpdqHash]:
    """videos: sequence of uint8[n_i,h,w] / uint8[n_i,h,w,3] arrays with one common frame
    geometry. All frames go through the PDQ kernels in one batch; per video the frames with
    quality >= 31 are kept in order (VideoHasher.finish semantics, vpdqpy/vpdqpy.py:119).
    autocrop: True or a dict of black_level / min_bright: every video is hashed inside its content rectangle
    (vpdq.hash_frames_autocrop). A dict of bar_color / bar_level / min_bright (vpdq.autocrop_rule) leaves out
    bars of the video's colour instead; an array bar_color has one row per video of `videos`. A dict of
    detail (True) / detail_level / min_detail leaves out smooth bars of any colour -- blurred, gradient -- (DESIGN 4.16)."""
    crop = vpdq.autocrop_rule(autocrop)
    videos = [np.ascontiguousarray(v, dtype=np.uint8) for v in videos]
    if not videos:
        return []
    shape = videos[0].shape[1:]
    for v in videos:
        if v.shape[1:] != shape:
            raise ValueError("all videos must share one frame geometry")
    lengths = np.array([v.shape[0] for v in videos], dtype=np.int64)
    if lengths.sum() == 0:
        return [vpdq.VpdqHash(b"") for _ in videos]
    flat = np.concatenate([v for v in videos if v.shape[0]], axis=0)
    if crop is not None:
        hashes, quality, _ = vpdq.hash_frames_autocrop(flat, np.concatenate([[0], np.cumsum(lengths)]), **crop.kwargs())
    else:
        hashes, quality = vpdq.hash_frames(flat)
    out, pos = [], 0
    for n in lengths:
        h, q = hashes[pos : pos + n], quality[pos : pos + n]
        out.append(vpdq.VpdqHash(h[q >= vpdq.QUALITY_TOLERANCE].tobytes()))
        pos += n
    return out


def dedupe_videos(videos, threshold: float = 50.0, policy: str | None = None):
    """Frames in, duplicate pairs out: (phashes, pairs) with pairs = sorted index pairs (a<b) the
    reference would mark as potential duplicates at `threshold` (dedup.py:445-502)."""
    phashes = hash_videos(videos)
    return phashes, search.find_potential_duplicates(phashes, threshold, policy)


# ------------------------------------------------------------------ device-resident form ------


class _DeviceScope:
    """The DeviceBuffers of one call. `temp` buffers (scratch, staging, uploaded operands) are freed on the way out, in the
    order they were registered; `keep` buffers are the call's results and are freed only if it raises -- after one
    hvd_dev_sync, since nothing may still run on a buffer that is freed. None is accepted and ignored (no scratch needed)."""

    def __init__(self):
        self._temp, self._kept = [], []

    def temp(self, buf):
        self._temp.append(buf)
        return buf

    def keep(self, buf):
        self._kept.append(buf)
        return buf

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            _lib.ensure().hvd_dev_sync()
        for b in self._temp + (self._kept if exc_type is not None else []):
            if b is not None:
                b.free()


def _stage_timer(timings):
    """timed(key, fn) -> fn(); with a timings dict, timings[key] = HIP-event time of fn's work on the library stream."""
    def timed(key, fn):
        if timings is None:
            return fn()
        lib = _lib.ensure()
        _lib.check(lib.hvd_timer_start())
        out = fn()
        ms = C.c_float(0)
        _lib.check(lib.hvd_timer_stop(C.byref(ms)))
        timings[key] = float(ms.value)
        return out

    return timed


def _hash_frames(entry, hash_bytes: int, d_frames_ptr: int, n: int, h: int, w: int, channels: int):
    """entry: hvd_dev_pdq_hash_frames or its dihedral form; hash_bytes: what it writes per frame."""
    lib = _lib.ensure()
    with _DeviceScope() as scope:
        d_h = scope.keep(DeviceBuffer(hash_bytes * max(n, 1)))
        d_q = scope.keep(DeviceBuffer(4 * max(n, 1)))
        sb = C.c_size_t(0)
        _lib.check(lib.hvd_pdq_scratch_bytes(n, h, w, channels, C.byref(sb)))
        d_s = scope.temp(DeviceBuffer(sb.value) if sb.value else None)
        _lib.check(entry(d_frames_ptr, n, h, w, channels, d_s.ptr if d_s else None, d_h.ptr, d_q.ptr))
        if d_s is not None:
            _lib.check(lib.hvd_dev_sync())  # the scratch must outlive the kernels
    return d_h, d_q


def hash_frames_on_device(d_frames_ptr: int, n: int, h: int, w: int, channels: int):
    """PDQ-hash n frames that already sit in HBM -> (d_hashes, d_quality) DeviceBuffers (n*32 B, int32[n]).
    Enqueued on the library stream; no host synchronisation."""
    return _hash_frames(_lib.ensure().hvd_dev_pdq_hash_frames, 32, d_frames_ptr, n, h, w, channels)


def hash_frames_dihedral_on_device(d_frames_ptr: int, n: int, h: int, w: int, channels: int):
    """Dihedral form of `hash_frames_on_device`: -> (d_hashes8, d_quality) DeviceBuffers (n*8*32 B in vpdq.TRANSFORMS
    order, int32[n]). Strict DCT mode only: the fma mode raises HvdError(HVD_ERR_STATE) before anything is launched."""
    lib = _lib.ensure()
    if lib.hvd_get_pdq_dct_mode() != 0:
        raise _lib.HvdError(_lib.HVD_ERR_STATE, "dihedral hashing has no fma DCT mode: set_dct_mode('strict') first")
    return _hash_frames(lib.hvd_dev_pdq_hash_frames_dihedral, 256, d_frames_ptr, n, h, w, channels)


def hash_frames_autocrop_on_device(d_frames_ptr: int, n: int, h: int, w: int, channels: int, offsets: np.ndarray,
                                   black_level: int = 16, min_bright: int = 1, timed=None, bar_color=None, bar_level=None,
                                   detail=False, detail_level=None, min_detail=None):
    """Content-rectangle form of `hash_frames_on_device`: the n frames in HBM are the videos of the CSR
    `offsets` (int64[V+1], from 0 to n); hvd_dev_content_rects finds every video's rectangle, hvd_dev_pdq_hash_frames_rects
    hashes every frame inside it. -> (d_hashes, d_quality, d_rects) DeviceBuffers (n*32 B, int32[n], int32[V,4]).
    timed(key, fn): optional stage timer, called with "rects_ms" and "hash_ms".
    bar_color ("auto", an int, a 3-tuple or an array [V, channels]) with bar_level (default 16): the rectangles leave out
    bars of the video's colour (hvd_dev_bar_colors where "auto", then hvd_dev_content_rects_color; both inside
    "rects_ms"); black_level then stays at its default.
    detail=True with detail_level / min_detail (defaults 8 and 8, unverified): the rectangles leave out smooth bars of any
    colour (hvd_dev_content_rects_detail in "rects_ms"); the other rules' keywords then stay at their defaults."""
    rule = vpdq.rect_rule(black_level, min_bright, bar_color, bar_level, detail, detail_level, min_detail)
    lib = _lib.ensure()
    offsets = _check_raw_offsets(offsets, n)
    V = offsets.size - 1
    run = timed if timed is not None else (lambda key, fn: fn())
    packed = vpdq._pack_bar_color(rule.colour, V, channels) if rule.kind == "color" else None
    with _DeviceScope() as scope:
        d_off = scope.keep(DeviceBuffer.from_array(offsets))
        d_r = scope.keep(DeviceBuffer(16 * max(V, 1)))
        vpdq.enqueue_rects(lib, rule, packed, d_frames_ptr, n, h, w, channels, d_off.ptr, V, d_r.ptr, scope.temp,
                           lambda fn: run("rects_ms", fn))
        d_h = scope.keep(DeviceBuffer(32 * max(n, 1)))
        d_q = scope.keep(DeviceBuffer(4 * max(n, 1)))
        sb = C.c_size_t(0)
        _lib.check(lib.hvd_pdq_rects_scratch_bytes(n, h, w, channels, C.byref(sb)))
        d_s = scope.temp(DeviceBuffer(sb.value) if sb.value else None)
        run("hash_ms", lambda: _lib.check(lib.hvd_dev_pdq_hash_frames_rects(d_frames_ptr, n, h, w, channels, d_off.ptr, V,
                                                                            d_r.ptr, d_s.ptr if d_s else None, d_h.ptr,
                                                                            d_q.ptr)))
        _lib.check(lib.hvd_dev_sync())  # the scratch and the offsets must outlive the kernels
        scope.temp(d_off)  # (done with: it goes after the scratch)
    return d_h, d_q, d_r


def hash_frames_crops_on_device(d_frames_ptr: int, n: int, h: int, w: int, channels: int, crops="aspect",
                                crop_quality: bool = True):
    """Crop-ladder form of `hash_frames_on_device`: -> (d_hashes8, d_quality, d_crop_quality, names)
    DeviceBuffers (n*8*32 B in the dihedral layout: slot 0 the full frame, slots 1..K the crops of
    vpdq.crop_ladder(h, w, crops) in list order, the rest zero; int32[n], the full frame's quality; int32[n*8] per slot) and
    the crops' names. crop_quality=False: the per-slot qualities are not written and d_crop_quality is None. Enqueued on the
    library stream; the scratch is freed after one hvd_dev_sync."""
    lib = _lib.ensure()
    names, rects = vpdq.crop_ladder(h, w, crops)
    K = len(names)
    with _DeviceScope() as scope:
        d_h = scope.keep(DeviceBuffer(256 * max(n, 1)))
        d_q = scope.keep(DeviceBuffer(4 * max(n, 1)))
        d_cq = scope.keep(DeviceBuffer(32 * max(n, 1))) if crop_quality else None
        sb = C.c_size_t(0)
        _lib.check(lib.hvd_pdq_crops_scratch_bytes(n, h, w, K, C.byref(sb)))
        d_s = scope.temp(DeviceBuffer(max(sb.value, 1)))
        _lib.check(lib.hvd_dev_pdq_hash_frames_crops(d_frames_ptr, n, h, w, channels, rects.ctypes.data, K, d_s.ptr, d_h.ptr,
                                                     d_q.ptr, d_cq.ptr if d_cq else None))
        _lib.check(lib.hvd_dev_sync())  # the scratch must outlive the kernels
    return d_h, d_q, d_cq, names


def transform_mask(names) -> int:
    """Transform names (search.transform_set) -> the mask of hvd_dev_compact_kept_dihedral (bit t = vpdq.TRANSFORMS[t])."""
    return sum(1 << vpdq.TRANSFORMS.index(t) for t in names)


def _check_raw_offsets(raw_offsets, n: int | None = None) -> np.ndarray:
    raw_offsets = np.ascontiguousarray(raw_offsets, dtype=np.int64)
    V = raw_offsets.size - 1
    if (V < 0 or raw_offsets[0] != 0 or (n is not None and raw_offsets[-1] != n) or (np.diff(raw_offsets) < 0).any()):
        raise ValueError("raw_offsets must be a CSR over the n frames")
    return raw_offsets


def _compaction_buffers(scope: _DeviceScope, raw_offsets: np.ndarray, n: int):
    """What both compactions take: the raw CSR, uploaded for the length of the scope, and their outputs for at most n kept
    frames. -> (d_raw_offsets, d_hashes, d_offsets, d_video)."""
    d_roff = scope.temp(DeviceBuffer.from_array(raw_offsets))
    return (d_roff, scope.keep(DeviceBuffer(32 * max(n, 1))), scope.keep(DeviceBuffer(8 * raw_offsets.size)),
            scope.keep(DeviceBuffer(4 * max(n, 1))))


def _default_max_dist(max_dist: int | None) -> int:
    return vpdq.frame_max_dist(search.DISTANCE_TOLERANCE) if max_dist is None else int(max_dist)


# What DeviceLibrary.ingest returns: the union library with its spread attached, the records with at least one
# new video (union numbering), the frames the common-frame rule dropped per video of the union.
Ingest = namedtuple("Ingest", "library records dropped")


class DeviceLibrary:
    """A video library resident in HBM: kept frame hashes (CSR by video), their FP4 image and the
    frame -> video map -- the operand of the video-level search."""

    def __init__(self, d_hashes: DeviceBuffer, d_offsets: DeviceBuffer, d_video: DeviceBuffer, n_frames: int,
                 n_videos: int):
        self.d_hashes, self.d_offsets, self.d_video = d_hashes, d_offsets, d_video
        self.n_frames, self.n_videos = int(n_frames), int(n_videos)
        self.d_img = None
        self.d_positions = None  # int32 per kept frame: its raw index inside its video (from_raw_hashes(positions=True))
        self._position_limit = 0
        self._lengths = None
        self.d_spread = None  # int32 per kept frame: the spread `attach_spread` (or `ingest`) left, at spread_max_dist
        self.spread_max_dist = None
        self.d_weights = None  # int32 per kept frame: the frames it stands for in the weighted search (`attach_weights`)

    @classmethod
    def from_raw_hashes(cls, d_hashes_ptr: int, d_quality_ptr: int, n: int, raw_offsets: np.ndarray,
                        min_quality: int = vpdq.QUALITY_TOLERANCE, positions: bool = False) -> "DeviceLibrary":
        """Quality filter + CSR on the device (hvd_dev_compact_kept). raw_offsets: int64[V+1] over the n
        hashed frames (host array; V+1 numbers are the only thing uploaded). positions=True: also the raw index inside
        its video of every kept frame (hvd_dev_kept_positions; the quality array is the caller's and may be gone later), the
        timeline `align` then works on; the default runs exactly the launches of the plain pipeline."""
        lib = _lib.ensure()
        raw_offsets = _check_raw_offsets(raw_offsets, n)
        V = raw_offsets.size - 1
        kept = C.c_int64(0)
        with _DeviceScope() as scope:
            d_roff, d_out_h, d_out_off, d_out_vid = _compaction_buffers(scope, raw_offsets, n)
            _lib.check(lib.hvd_dev_compact_kept(d_hashes_ptr, d_quality_ptr, n, d_roff.ptr, V, int(min_quality),
                                                d_out_h.ptr, d_out_off.ptr, d_out_vid.ptr, C.byref(kept)))
            d_pos = None
            if positions:
                d_pos = scope.keep(DeviceBuffer(4 * max(n, 1)))
                _lib.check(lib.hvd_dev_kept_positions(d_quality_ptr, n, d_roff.ptr, V, int(min_quality), d_pos.ptr))
                _lib.check(lib.hvd_dev_sync())  # the raw offsets are freed on the way out
        library = cls(d_out_h, d_out_off, d_out_vid, kept.value, V)
        library.d_positions = d_pos
        library._position_limit = int(np.diff(raw_offsets).max()) if V else 0  # every position is below this
        return library

    @classmethod
    def from_raw_dihedral(cls, d_hashes8_ptr: int, d_quality_ptr: int, n: int, raw_offsets: np.ndarray, transforms,
                          min_quality: int = vpdq.QUALITY_TOLERANCE) -> tuple["DeviceLibrary", "DeviceQueries | None"]:
        """Quality filter + CSR of the dihedral hashes (hvd_dev_compact_kept_dihedral). transforms: names as
        search.transform_set returns them (identity included). -> (identity library, the same as from_raw_hashes on the
        plain hashes; query set of the other variants, None when there are none)."""
        return cls._from_raw_slots(d_hashes8_ptr, d_quality_ptr, n, raw_offsets, transform_mask(transforms),
                                   tuple(t for t in transforms if t != "identity"), min_quality)

    @classmethod
    def from_raw_crops(cls, d_hashes8_ptr: int, d_quality_ptr: int, n: int, raw_offsets: np.ndarray, names,
                       min_quality: int = vpdq.QUALITY_TOLERANCE) -> tuple["DeviceLibrary", "DeviceQueries | None"]:
        """from_raw_dihedral for the crop-ladder hashes (hvd_dev_pdq_hash_frames_crops writes the dihedral layout: slot 0
        the full frame, slot k + 1 crop names[k]): the same compaction with the slot mask (1 << (K + 1)) - 1. -> (identity
        library; query set whose `transforms` are the crops' names, query video v * K + k for names[k])."""
        names = tuple(names)
        return cls._from_raw_slots(d_hashes8_ptr, d_quality_ptr, n, raw_offsets, (1 << (len(names) + 1)) - 1, names, min_quality)

    @classmethod
    def _from_raw_slots(cls, d_hashes8_ptr: int, d_quality_ptr: int, n: int, raw_offsets: np.ndarray, mask: int, cross: tuple,
                        min_quality: int):
        """hvd_dev_compact_kept_dihedral with a slot mask (bit t = slot t of the 8 hashes per frame, bit 0 set): the identity
        library from slot 0, the query set from the other set bits in ascending order, named by `cross`."""
        lib = _lib.ensure()
        raw_offsets = _check_raw_offsets(raw_offsets, n)
        V = raw_offsets.size - 1
        K = len(cross)
        kept = C.c_int64(0)
        with _DeviceScope() as scope:
            d_roff, d_out_h, d_out_off, d_out_vid = _compaction_buffers(scope, raw_offsets, n)
            d_qh, d_qv, d_qx = (scope.keep(DeviceBuffer(size * K * max(n, 1))) if K else None for size in (32, 4, 4))
            _lib.check(lib.hvd_dev_compact_kept_dihedral(
                d_hashes8_ptr, d_quality_ptr, n, d_roff.ptr, V, int(min_quality), int(mask), d_out_h.ptr,
                d_out_off.ptr, d_out_vid.ptr, d_qh.ptr if K else None, d_qv.ptr if K else None, d_qx.ptr if K else None,
                C.byref(kept)))
        library = cls(d_out_h, d_out_off, d_out_vid, kept.value, V)
        queries = DeviceQueries(d_qh, d_qv, d_qx, K * kept.value, K * V, tuple(cross)) if K else None
        return library, queries

    @classmethod
    def from_host(cls, frames: np.ndarray, offsets: np.ndarray) -> "DeviceLibrary":
        """Upload an existing library (hashes uint8[sum,32] + CSR offsets)."""
        lib = _lib.ensure()
        frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, 32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n, V = frames.shape[0], offsets.size - 1
        if V < 0 or offsets[-1] != n:
            raise ValueError("offsets[-1] must equal the number of frame hashes")
        d_h = DeviceBuffer.from_array(frames) if n else DeviceBuffer(1)
        d_off = DeviceBuffer.from_array(offsets)
        d_vid = DeviceBuffer(4 * max(n, 1))
        _lib.check(lib.hvd_dev_video_of_frames(d_off.ptr, V, n, d_vid.ptr))
        return cls(d_h, d_off, d_vid, n, V)

    def image(self) -> DeviceBuffer:
        """FP4 image of the kept hashes (built once, cached)."""
        if self.d_img is None:
            lib = _lib.ensure()
            sz = C.c_size_t(0)
            _lib.check(lib.hvd_fp4_image_bytes(self.n_frames, C.byref(sz)))
            self.d_img = DeviceBuffer(sz.value)
            _lib.check(lib.hvd_dev_expand_fp4(self.d_hashes.ptr, self.n_frames, self.d_img.ptr))
        return self.d_img

    def offsets(self) -> np.ndarray:
        return self.d_offsets.to_array(np.int64, self.n_videos + 1)

    def lengths(self) -> np.ndarray:
        if self._lengths is None:
            self._lengths = np.diff(self.offsets())
        return self._lengths

    def hashes(self) -> np.ndarray:
        return self.d_hashes.to_array(np.uint8, 32 * self.n_frames).reshape(-1, 32)

    def attach_weights(self, d_weights: DeviceBuffer) -> DeviceBuffer:
        """Give every kept frame a weight for `match_videos(weighted=True)`: d_weights holds one int32 per frame,
        each at least 1 -- the runs buffer of `without_repeated_frames` as it is. The buffer becomes this library's: `free`
        frees it, and weights attached earlier are freed here. Nothing is checked on the device; `weight_totals` refuses a
        video whose total the uint32 counters cannot hold. -> the buffer."""
        if d_weights.nbytes < 4 * self.n_frames:
            raise ValueError("weights must hold one int32 per kept frame")
        if self.d_weights is not None and self.d_weights is not d_weights:
            self.d_weights.free()
        self.d_weights = d_weights
        return d_weights

    def _check_unweighted(self, what: str) -> None:
        if self.d_weights is not None:
            raise ValueError(f"{what} would drop the attached weights: it is not defined on a weighted library")

    def weight_totals(self, max_weight: int = 0) -> np.ndarray:
        """hvd_dev_video_weights: int64[V], per video the sum of min(weight, max_weight) over its frames (max_weight 0: of the
        weights) -- what stands for `lengths()` after a weighted search. V numbers cross PCIe. ValueError: a total above
        2^32 - 1, which the uint32 counters of that video's records cannot hold."""
        if self.d_weights is None:
            raise ValueError("no weights attached: call attach_weights first")
        max_weight = search.check_max_weight(max_weight)
        lib = _lib.ensure()
        V = self.n_videos
        if V == 0:
            return np.zeros(0, dtype=np.int64)
        with _DeviceScope() as scope:
            d_totals = scope.temp(DeviceBuffer(8 * V))
            _lib.check(lib.hvd_dev_video_weights(self.d_weights.ptr, self.d_offsets.ptr, V, self.n_frames, max_weight, d_totals.ptr))
            totals = d_totals.to_array(np.int64, V)
        over = np.flatnonzero(totals > search.WEIGHT_TOTAL_LIMIT)
        if over.size:
            raise ValueError(f"video {int(over[0])}: capped weight total {int(totals[over[0]])} exceeds 2^32 - 1")
        return totals

    def match_videos(self, max_dist: int | None = None, rank: int = 0, world: int = 1, cap: int | None = None,
                     weighted: bool = False, max_weight: int = 0) -> np.ndarray:
        """hvd_dev_vpdq_match_videos: VMATCH_DTYPE records sorted by (a, b); only these cross PCIe. weighted=True:
        hvd_dev_vpdq_match_videos_weighted with the attached weights -- a matched frame adds
        min(weight, max_weight) (max_weight 0: its weight) to q_hits / t_hits instead of 1, `weight_totals(max_weight)` are
        the denominators; on this context alone (world must be 1)."""
        if weighted:
            if world != 1 or rank != 0:
                raise ValueError("the weighted search is not sharded over a device group: world must be 1")
            if self.d_weights is None:
                raise ValueError("no weights attached: call attach_weights first")
            max_weight = search.check_max_weight(max_weight)
        elif max_weight:
            raise ValueError("max_weight caps weights: pass weighted=True as well")
        return self._match(None, None, weighted, max_weight, max_dist, rank, world, cap)

    def _match(self, queries: "DeviceLibrary | None", excl, weighted: bool, max_weight: int, max_dist, rank: int, world: int,
               cap) -> np.ndarray:
        """The device video search behind match_videos, match_queries and match_library. queries: the query side,
        this library being the target side -- None: the symmetric search of this library; excl: the exclusion maps (query
        side's, this side's) as DeviceBuffers, or None; weighted: the attached weights (symmetric only). Nothing to compare:
        no call. Default cap: max(4096, videos of the query side). The images are built inside the launch, after the record
        buffers, the query side's first."""
        lib = _lib.ensure()
        max_dist = _default_max_dist(max_dist)
        q = self if queries is None else queries
        if max_dist < 0 or (self.n_frames < 2 if queries is None else queries.n_frames == 0 or self.n_frames == 0):
            return np.zeros(0, dtype=VMATCH_DTYPE)
        excl_q, excl_t = (None, None) if excl is None else (excl[0].ptr, excl[1].ptr)

        def launch(d_out, cap_, d_cnt):
            if queries is not None:
                return lib.hvd_dev_vpdq_match_videos_cross(q.image().ptr, q.n_frames, q.d_video.ptr, excl_q, self.image().ptr,
                                                           self.n_frames, self.d_video.ptr, excl_t, max_dist, rank, world, d_out,
                                                           cap_, d_cnt)
            if weighted:
                return lib.hvd_dev_vpdq_match_videos_weighted(q.image().ptr, q.n_frames, q.d_video.ptr, self.d_weights.ptr,
                                                              max_weight, max_dist, d_out, cap_, d_cnt)
            return lib.hvd_dev_vpdq_match_videos(q.image().ptr, q.n_frames, q.d_video.ptr, max_dist, rank, world, d_out, cap_, d_cnt)

        return _search_records(launch, max(4096, q.n_videos) if cap is None else int(cap))

    def match_queries(self, queries: "DeviceQueries", max_dist: int | None = None, rank: int = 0, world: int = 1,
                      cap: int | None = None) -> np.ndarray:
        """hvd_dev_vpdq_match_videos_cross of a query set (from_raw_dihedral) against this library, a video never against
        its own variants (the library's frame -> video map is the target's exclusion map). VMATCH_DTYPE records (a = query
        video v*K + k, b = video) sorted by (a, b); the same record buffer, cap and emit-again retry as match_videos."""
        if queries is None:
            return np.zeros(0, dtype=VMATCH_DTYPE)
        return self._match(queries, (queries.d_excl, self.d_video), False, 0, max_dist, rank, world, cap)

    def positions(self) -> np.ndarray | None:
        return None if self.d_positions is None else self.d_positions.to_array(np.int32, self.n_frames)

    def align(self, records, slack: int = search.ALIGN_SLACK, max_dist: int | None = None) -> np.ndarray:
        """hvd_dev_vpdq_align_videos of the listed pairs of this library against itself (records: VMATCH records, or
        int[M, 2]): one VALIGN_DTYPE record per pair, in their order. The hashes, the CSR and the positions stay where they
        are; the pair list goes up, the records come back. Positions: those of from_raw_hashes(positions=True), else the
        index inside the kept video."""
        return self._align(records, search.AlignMode(), slack, max_dist)

    def align_segments(self, records, slack: int = search.ALIGN_SLACK, max_dist: int | None = None,
                       max_segments: int = _lib.ALIGN_MAX_SEGMENTS, min_band_votes: int = 1) -> np.ndarray:
        """hvd_dev_vpdq_align_segments of the listed pairs of this library against itself: one VSEGMENTS_DTYPE record per
        pair, in their order (search.align_segments on what is in HBM; operands and positions as `align`)."""
        return self._align(records, search.AlignMode(None, max_segments, min_band_votes), slack, max_dist)

    def align_rates(self, records, rates=search.DEFAULT_RATES, slack: int = search.ALIGN_SLACK,
                    max_dist: int | None = None) -> np.ndarray:
        """hvd_dev_vpdq_align_rates of the listed pairs of this library against itself: one VRATE_DTYPE record per pair, in
        their order (search.align_rates on what is in HBM; operands and positions as `align`). A broken rate list gives
        INT32_MIN records, as the device entry does."""
        return self._align(records, search.AlignMode(rates), slack, max_dist)

    def align_rate_segments(self, records, rates=search.DEFAULT_RATES, slack: int = search.ALIGN_SLACK,
                            max_dist: int | None = None, max_segments: int = _lib.ALIGN_MAX_SEGMENTS,
                            min_band_votes: int = 1) -> np.ndarray:
        """hvd_dev_vpdq_align_rate_segments of the listed pairs of this library against itself: one VRSEGMENTS_DTYPE record
        per pair, in their order (search.align_rate_segments on what is in HBM; operands and positions as `align`). A broken
        rate list gives INT32_MIN records, as the device entry does."""
        return self._align(records, search.AlignMode(rates, max_segments, min_band_votes), slack, max_dist)

    def align_signed(self, records, rates=search.REVERSED_RATES, slack: int = search.ALIGN_SLACK,
                     max_dist: int | None = None, max_segments: int = _lib.ALIGN_MAX_SEGMENTS,
                     min_band_votes: int = 1) -> np.ndarray:
        """hvd_dev_vpdq_align_signed of the listed pairs of this library against itself: one VSSEGMENTS_DTYPE record per
        pair, in their order (search.align_signed on what is in HBM; operands and positions as `align`). A list that is not
        sound as a signed list gives INT32_MIN records, as the device entry does."""
        return self._align(records, search.AlignMode(rates, max_segments, min_band_votes, True), slack, max_dist)

    def align_loops(self, records, rates=search.REVERSED_RATES, slack: int = search.ALIGN_SLACK, max_dist: int | None = None,
                    max_rounds: int = _lib.ALIGN_MAX_ROUNDS, min_band_votes: int = 1) -> np.ndarray:
        """hvd_dev_vpdq_align_loops of the listed pairs of this library against itself: one VLOOPS_DTYPE record per pair, in
        their order (search.align_loops on what is in HBM; operands and positions as `align`). The loop is a pair's a side:
        list (b, a) as well to try the other orientation. A list that is not sound as a signed list gives INT32_MIN records,
        as the device entry does."""
        return self._align(records, search.AlignMode(rates, max_rounds, min_band_votes, True, True), slack, max_dist)

    def _align(self, records, mode: search.AlignMode, slack, max_dist) -> np.ndarray:
        """One device-resident alignment call over this library against itself: the entries, the record dtype and the extra
        arguments are those of the mode's row (search.ALIGN_ROWS)."""
        lib = _lib.ensure()
        row = mode.row
        rates = None if mode.rates is None else search.rate_array(mode.rates)
        pairs = search.pair_array(records)
        M = pairs.shape[0]
        max_dist = _default_max_dist(max_dist)
        out = np.zeros(M, dtype=row.dtype)
        out["a"], out["b"] = pairs[:, 0], pairs[:, 1]
        if M == 0 or max_dist < 0:
            return out
        # the scratch serves the widest pair this library can hold: positions lie below the longest (raw) video's length
        if self.d_positions is None:
            lengths = self.lengths()
            limit = int(lengths.max()) if lengths.size else 0
        else:
            limit = self._position_limit
        # a pair's histogram is sized by its largest bins_r = |num| span_a + den span_b + 1 + 2 slack max(|num|, den), slope one
        # among them (a signed mode lists negative nums)
        max_bins = max((abs(num) + den) * (max(limit, 1) - 1) + 1 + 2 * int(slack) * max(abs(num), den)
                       for num, den in [(1, 1)] + ([] if rates is None else rates.tolist()))
        sb = C.c_size_t(0)
        _lib.check(getattr(lib, row.scratch_entry)(min(max_bins, _lib.ALIGN_MAX_BINS), C.byref(sb)))
        with _DeviceScope() as scope:
            d_pairs = scope.temp(DeviceBuffer.from_array(pairs))
            d_out = scope.temp(DeviceBuffer(row.dtype.itemsize * M))
            d_scr = scope.temp(DeviceBuffer(sb.value) if sb.value else None)
            d_pos = self.d_positions.ptr if self.d_positions is not None else None
            _lib.check(getattr(lib, row.device_entry)(
                self.d_hashes.ptr, self.d_offsets.ptr, self.n_videos, d_pos, self.d_hashes.ptr, self.d_offsets.ptr, self.n_videos,
                d_pos, d_pairs.ptr, M, max_dist, int(slack), *mode.entry_args(rates), d_scr.ptr if d_scr else None, sb.value, d_out.ptr))
            aligned = d_out.to_array(row.dtype, M)  # (the copy waits for the library stream)
            lib.hvd_dev_sync()  # nothing may still run on a buffer that is freed here
        return aligned

    def cover(self, records, slack: int = search.ALIGN_SLACK, max_dist: int | None = None,
              min_aligned: int = 4) -> tuple[np.ndarray, np.ndarray]:
        """hvd_dev_vpdq_cover_videos of the listed pairs of this library against itself (records: VMATCH records, or
        int[M, 2]; search.cover_videos on what is in HBM): -> (one VALIGN_DTYPE record per pair, in their order -- `align`'s,
        word for word; one VCOVER_DTYPE record per video: the union of its aligned frames over all its pairs). The union is
        taken in a bitmap on the device; the pair list goes up, the records come back. Operands and positions as `align`."""
        lib = _lib.ensure()
        pairs = search.pair_array(records)
        M, V = pairs.shape[0], self.n_videos
        max_dist = _default_max_dist(max_dist)
        aligned = np.zeros(M, dtype=_lib.VALIGN_DTYPE)
        aligned["a"], aligned["b"] = pairs[:, 0], pairs[:, 1]
        if V == 0:
            return aligned, np.zeros(0, dtype=_lib.VCOVER_DTYPE)
        if max_dist < 0:
            cover = np.zeros(V, dtype=_lib.VCOVER_DTYPE)
            cover["frames"] = self.lengths()
            return aligned, cover
        # the scratch serves the widest pair this library can hold, as `_align` sizes it, and the bitmap over its frames
        if self.d_positions is None:
            lengths = self.lengths()
            limit = int(lengths.max()) if lengths.size else 0
        else:
            limit = self._position_limit
        max_bins = 2 * (max(limit, 1) - 1) + 1 + 2 * int(slack)
        sb = C.c_size_t(0)
        _lib.check(lib.hvd_cover_scratch_bytes(self.n_frames, min(max_bins, _lib.ALIGN_MAX_BINS), C.byref(sb)))
        with _DeviceScope() as scope:
            d_pairs = scope.temp(DeviceBuffer.from_array(pairs) if M else None)
            d_out = scope.temp(DeviceBuffer(_lib.VALIGN_DTYPE.itemsize * M) if M else None)
            d_cover = scope.temp(DeviceBuffer(_lib.VCOVER_DTYPE.itemsize * V))
            d_scr = scope.temp(DeviceBuffer(sb.value) if sb.value else None)
            d_pos = self.d_positions.ptr if self.d_positions is not None else None
            _lib.check(lib.hvd_dev_vpdq_cover_videos(
                self.d_hashes.ptr, self.d_offsets.ptr, V, self.n_frames, d_pos, d_pairs.ptr if M else None, M, max_dist, int(slack),
                int(min_aligned), d_scr.ptr if d_scr else None, sb.value, d_out.ptr if M else None, d_cover.ptr))
            if M:
                aligned = d_out.to_array(_lib.VALIGN_DTYPE, M)  # (the copy waits for the library stream)
            cover = d_cover.to_array(_lib.VCOVER_DTYPE, V)
            lib.hvd_dev_sync()  # nothing may still run on a buffer that is freed here
        return aligned, cover

    def spread(self, max_dist: int | None = None) -> DeviceBuffer:
        """hvd_dev_vpdq_frame_spread: int32 per kept frame, the number of OTHER videos of this library the frame occurs in
        (DESIGN 4.13), as a DeviceBuffer that is the caller's to free. The compare and the key set of `match_videos`
        without its fold; the records of the last search stay valid for hvd_dev_vpdq_emit_again."""
        with _DeviceScope() as scope:
            d_spread = scope.keep(DeviceBuffer(4 * max(self.n_frames, 1)))
            if not self._spread_into(None, max_dist, False, d_spread.ptr, None):
                d_spread.zero()
        return d_spread

    def _spread_into(self, other: "DeviceLibrary | None", max_dist, accumulate: bool, sq_ptr, st_ptr) -> bool:
        """The device spread behind spread, spread_cross and ingest, into buffers of the caller's. other: the
        query side, this library being the target side -- None: the spread inside this library, into sq_ptr. accumulate
        (two sides): add to what the buffers hold. -> False: nothing to compare, nothing was called."""
        lib = _lib.ensure()
        max_dist = _default_max_dist(max_dist)
        if max_dist < 0 or (self.n_frames < 2 if other is None else other.n_frames == 0 or self.n_frames == 0):
            return False
        if other is None:
            _lib.check(lib.hvd_dev_vpdq_frame_spread(self.image().ptr, self.n_frames, self.d_video.ptr, max_dist, sq_ptr))
        else:
            _lib.check(lib.hvd_dev_vpdq_frame_spread_cross(other.image().ptr, other.n_frames, other.d_video.ptr, self.image().ptr,
                                                           self.n_frames, self.d_video.ptr, max_dist, int(accumulate), sq_ptr,
                                                           st_ptr))
        return True

    def without_common_frames(self, max_videos: int, max_share: int = 50,
                              max_dist: int | None = None) -> tuple["DeviceLibrary", np.ndarray]:
        """This library without the frames that many videos share (search.without_common_frames on what is in HBM): spread ->
        rule (hvd_dev_common_frames) -> compaction (hvd_dev_compact_kept on the keep flags, bound 1). -> (a NEW library,
        dropped int64[V]); this one is untouched and still the caller's to free. The result always has positions: this
        library's, gathered (hvd_dev_gather_kept_i32), else the index inside this library's video
        (hvd_dev_kept_positions) -- so `align*` work on the timeline they had before. Attached weights are gathered likewise.
        Nothing but CSR offsets crosses PCIe."""
        max_videos, max_share = search.check_common_rule(max_videos, max_share)
        lib = _lib.ensure()
        n, V = self.n_frames, self.n_videos
        kept = C.c_int64(0)
        with _DeviceScope() as scope:
            d_spread = scope.temp(self.spread(max_dist))
            d_keep = scope.temp(DeviceBuffer(4 * max(n, 1)))
            _lib.check(lib.hvd_dev_common_frames(d_spread.ptr, self.d_offsets.ptr, V, n, max_videos, max_share, d_keep.ptr))
            d_h, d_vid, d_pos = (scope.keep(DeviceBuffer(size * max(n, 1))) for size in (32, 4, 4))
            d_off = scope.keep(DeviceBuffer(8 * (V + 1)))
            _lib.check(lib.hvd_dev_compact_kept(self.d_hashes.ptr, d_keep.ptr, n, self.d_offsets.ptr, V, 1, d_h.ptr, d_off.ptr,
                                                d_vid.ptr, C.byref(kept)))
            if self.d_positions is not None:
                _lib.check(lib.hvd_dev_gather_kept_i32(self.d_positions.ptr, d_keep.ptr, n, d_pos.ptr))
            else:
                _lib.check(lib.hvd_dev_kept_positions(d_keep.ptr, n, self.d_offsets.ptr, V, 1, d_pos.ptr))
            d_w = None
            if self.d_weights is not None:  # a kept frame keeps its weight
                d_w = scope.keep(DeviceBuffer(4 * max(n, 1)))
                _lib.check(lib.hvd_dev_gather_kept_i32(self.d_weights.ptr, d_keep.ptr, n, d_w.ptr))
            _lib.check(lib.hvd_dev_sync())  # the keep flags are freed on the way out
        library = DeviceLibrary(d_h, d_off, d_vid, kept.value, V)
        library.d_positions = d_pos
        library.d_weights = d_w
        lengths = self.lengths()
        library._position_limit = self._position_limit if self.d_positions is not None else \
            (int(lengths.max()) if lengths.size else 0)
        return library, (lengths - library.lengths()).astype(np.int64)

    def without_repeated_frames(self, max_dist: int, max_run: int = 0) -> tuple["DeviceLibrary", np.ndarray, DeviceBuffer]:
        """This library with every run of near-identical consecutive frames collapsed to its first frame
        (search.without_repeated_frames on what is in HBM): the rule (hvd_dev_frame_runs) -> compaction
        (hvd_dev_compact_kept on the keep flags, bound 1). -> (a NEW library, dropped int64[V], runs: a DeviceBuffer of one
        int32 per kept frame, the frames it stands for, the caller's to free); this one is untouched and still the caller's to
        free. The result always has positions, as `without_common_frames` makes them: this library's, gathered
        (hvd_dev_gather_kept_i32), else the index inside this library's video (hvd_dev_kept_positions); a kept frame carries
        the position of the first frame of its run. Nothing but CSR offsets crosses PCIe. ValueError on a library with
        attached weights: the runs of a second collapse would have to be sums of weights, which nothing computes."""
        self._check_unweighted("without_repeated_frames")
        max_dist, max_run = search.check_run_rule(max_dist, max_run)
        lib = _lib.ensure()
        n, V = self.n_frames, self.n_videos
        kept = C.c_int64(0)
        with _DeviceScope() as scope:
            d_keep, d_run = (scope.temp(DeviceBuffer(4 * max(n, 1))) for _ in range(2))
            if max_dist < 0:  # nothing can match: every frame is its own run, which is the rule at max_run 1
                max_dist, max_run = 0, 1
            _lib.check(lib.hvd_dev_frame_runs(self.d_hashes.ptr, self.d_offsets.ptr, V, n, max_dist, max_run, d_keep.ptr,
                                              d_run.ptr))
            d_h, d_vid, d_pos, d_runs = (scope.keep(DeviceBuffer(size * max(n, 1))) for size in (32, 4, 4, 4))
            d_off = scope.keep(DeviceBuffer(8 * (V + 1)))
            _lib.check(lib.hvd_dev_compact_kept(self.d_hashes.ptr, d_keep.ptr, n, self.d_offsets.ptr, V, 1, d_h.ptr, d_off.ptr,
                                                d_vid.ptr, C.byref(kept)))
            if self.d_positions is not None:
                _lib.check(lib.hvd_dev_gather_kept_i32(self.d_positions.ptr, d_keep.ptr, n, d_pos.ptr))
            else:
                _lib.check(lib.hvd_dev_kept_positions(d_keep.ptr, n, self.d_offsets.ptr, V, 1, d_pos.ptr))
            _lib.check(lib.hvd_dev_gather_kept_i32(d_run.ptr, d_keep.ptr, n, d_runs.ptr))
            _lib.check(lib.hvd_dev_sync())  # the keep flags and the run words are freed on the way out
        library = DeviceLibrary(d_h, d_off, d_vid, kept.value, V)
        library.d_positions = d_pos
        lengths = self.lengths()
        library._position_limit = self._position_limit if self.d_positions is not None else \
            (int(lengths.max()) if lengths.size else 0)
        return library, (lengths - library.lengths()).astype(np.int64), d_runs

    # ---- new files against this library ----

    def attach_spread(self, max_dist: int | None = None) -> DeviceBuffer:
        """`spread(max_dist)`, kept: d_spread / spread_max_dist carry it from call to call (`ingest` starts from it) and
        `free` frees it. -> the buffer, which stays this library's."""
        max_dist = _default_max_dist(max_dist)
        d_spread = self.spread(max_dist)
        if self.d_spread is not None:
            self.d_spread.free()
        self.d_spread, self.spread_max_dist = d_spread, max_dist
        return d_spread

    def spread_cross(self, other: "DeviceLibrary", max_dist: int | None = None) -> tuple[DeviceBuffer, DeviceBuffer]:
        """hvd_dev_vpdq_frame_spread_cross of `other` (the new batch, query side) against this library (target side):
        -> (sq, st), DeviceBuffers that are the caller's to free. sq: int32 per frame of `other`, the number of this library's
        videos it occurs in; st: int32 per frame of this library, the number of `other`'s videos it occurs in. The records of
        the last search stay valid for hvd_dev_vpdq_emit_again."""
        with _DeviceScope() as scope:
            d_sq = scope.keep(DeviceBuffer(4 * max(other.n_frames, 1)))
            d_st = scope.keep(DeviceBuffer(4 * max(self.n_frames, 1)))
            if not self._spread_into(other, max_dist, False, d_sq.ptr, d_st.ptr):
                d_sq.zero()
                d_st.zero()
        return d_sq, d_st

    def match_library(self, other: "DeviceLibrary", max_dist: int | None = None, cap: int | None = None) -> np.ndarray:
        """hvd_dev_vpdq_match_videos_cross of another resident library (query side) against this one (target side), no
        exclusion maps: VMATCH_DTYPE records (a = other's video, b = this library's video) sorted by (a, b); the same record
        buffer, cap and emit-again retry as match_queries."""
        return self._match(other, None, False, 0, max_dist, 0, 1, cap)

    def _check_extension(self, other: "DeviceLibrary") -> None:
        """ValueError unless `extended(other)` can be built; touches nothing on the device."""
        self._check_unweighted("extended / ingest")
        other._check_unweighted("extended / ingest")
        if (self.d_positions is None) != (other.d_positions is None):
            raise ValueError("positions on one side only: both libraries carry them or neither does")
        if self.n_frames + other.n_frames >= (1 << 32) - 1 or self.n_videos + other.n_videos >= (1 << 31):
            raise ValueError("the union is over the library limits: frames below 2^32 - 1, videos below 2^31")

    def extended(self, other: "DeviceLibrary") -> "DeviceLibrary":
        """The union U = this library || other as a NEW library: this library's videos keep their numbers, other's video v
        becomes n_videos + v, frames likewise. Both sources are untouched and stay the caller's. Device-to-device copies of
        the hashes (and positions: carried if both have them, absent if neither), a host-built CSR (V + 1 numbers go up),
        hvd_dev_video_of_frames for the map."""
        self._check_extension(other)
        lib = _lib.ensure()
        nT, nQ, VT = self.n_frames, other.n_frames, self.n_videos
        n, V = nT + nQ, VT + other.n_videos
        offsets = np.concatenate([self.offsets(), other.offsets()[1:] + nT]).astype(np.int64)
        with _DeviceScope() as scope:
            d_h = scope.keep(DeviceBuffer(32 * max(n, 1)))
            d_off = scope.keep(DeviceBuffer.from_array(offsets))
            d_vid = scope.keep(DeviceBuffer(4 * max(n, 1)))
            d_pos = scope.keep(DeviceBuffer(4 * max(n, 1))) if self.d_positions is not None else None
            for d_dst, src_t, src_q, size in ((d_h, self.d_hashes, other.d_hashes, 32), (d_pos, self.d_positions, other.d_positions, 4)):
                if d_dst is None:
                    continue
                if nT:
                    _lib.check(lib.hvd_memcpy_d2d(d_dst.ptr, src_t.ptr, size * nT))
                if nQ:
                    _lib.check(lib.hvd_memcpy_d2d(d_dst.ptr + size * nT, src_q.ptr, size * nQ))
            _lib.check(lib.hvd_dev_video_of_frames(d_off.ptr, V, n, d_vid.ptr))
            _lib.check(lib.hvd_dev_sync())  # the sources are the caller's to free from here on
        library = DeviceLibrary(d_h, d_off, d_vid, n, V)
        library.d_positions = d_pos
        library._position_limit = max(self._position_limit, other._position_limit)
        return library

    def _spread_at(self, max_dist: int, scope: _DeviceScope) -> DeviceBuffer:
        """The attached spread if it was taken at max_dist, else a fresh one that the scope frees."""
        if self.d_spread is not None and self.spread_max_dist == max_dist:
            return self.d_spread
        return scope.temp(self.spread(max_dist))

    def _kept_by(self, d_keep_ptr: int) -> "DeviceLibrary":
        """hvd_dev_compact_kept of this library on keep flags (bound 1): hashes, CSR and map of what is left; no positions."""
        lib = _lib.ensure()
        n, V = self.n_frames, self.n_videos
        kept = C.c_int64(0)
        with _DeviceScope() as scope:
            d_h, d_vid = (scope.keep(DeviceBuffer(size * max(n, 1))) for size in (32, 4))
            d_off = scope.keep(DeviceBuffer(8 * (V + 1)))
            _lib.check(lib.hvd_dev_compact_kept(self.d_hashes.ptr, d_keep_ptr, n, self.d_offsets.ptr, V, 1, d_h.ptr, d_off.ptr,
                                                d_vid.ptr, C.byref(kept)))
        return DeviceLibrary(d_h, d_off, d_vid, kept.value, V)

    def ingest(self, new: "DeviceLibrary", max_videos: int | None = None, max_share: int = 50,
               max_dist: int | None = None) -> Ingest:
        """A batch of new videos against this library, with the common-frame filter of DESIGN 4.13 over the union and without
        its O(n^2) passes over what was already there. U = this library || new (`extended`);
        spread_U = (spread_T + st) || (spread_Q + sq): this library's spread comes from `attach_spread` if it was taken at
        max_dist (else it is computed), new's likewise, and ONE hvd_dev_vpdq_frame_spread_cross call adds st and sq on top. With
        max_videos set, the rule (hvd_dev_common_frames) runs on U and each side is compacted by its slice of the keep flags.
        -> Ingest(library = U with spread_U attached: the next ingest starts from it; records = those of the video search on
        the filtered U that hold at least one new video (b >= this library's n_videos), in U's numbering, a < b, sorted by
        (a, b): new x old by `match_library`, new x new by `match_videos`; old x old pairs are neither re-judged nor returned;
        dropped int64[V_U]). max_videos=None: no frame is dropped. This library and `new` are untouched and stay the
        caller's; the result's library is the caller's to free."""
        if max_videos is not None:
            max_videos, max_share = search.check_common_rule(max_videos, max_share)
        else:
            search.check_common_rule(0, max_share)  # (unused without the rule, but never accepted broken)
        self._check_extension(new)
        lib = _lib.ensure()
        max_dist = _default_max_dist(max_dist)
        nT, nQ, VT, VQ = self.n_frames, new.n_frames, self.n_videos, new.n_videos
        n, V = nT + nQ, VT + VQ
        with _DeviceScope() as scope:
            union = scope.keep(self.extended(new))
            d_spread_t, d_spread_q = self._spread_at(max_dist, scope), new._spread_at(max_dist, scope)
            d_su = DeviceBuffer(4 * max(n, 1))
            union.d_spread, union.spread_max_dist = d_su, max_dist  # (freed with the union)
            if nT:
                _lib.check(lib.hvd_memcpy_d2d(d_su.ptr, d_spread_t.ptr, 4 * nT))
            if nQ:
                _lib.check(lib.hvd_memcpy_d2d(d_su.ptr + 4 * nT, d_spread_q.ptr, 4 * nQ))
            if not self._spread_into(new, max_dist, True, d_su.ptr + 4 * nT, d_su.ptr):
                _lib.check(lib.hvd_dev_sync())  # the copies read buffers the scope frees
            old, fresh = self, new
            dropped = np.zeros(V, dtype=np.int64)
            if max_videos is not None:
                d_keep = scope.temp(DeviceBuffer(4 * max(n, 1)))
                _lib.check(lib.hvd_dev_common_frames(d_su.ptr, union.d_offsets.ptr, V, n, max_videos, max_share, d_keep.ptr))
                old = scope.temp(self._kept_by(d_keep.ptr))
                fresh = scope.temp(new._kept_by(d_keep.ptr + 4 * nT))
                dropped = np.concatenate([self.lengths() - old.lengths(), new.lengths() - fresh.lengths()]).astype(np.int64)
            cross = old.match_library(fresh, max_dist)
            among = fresh.match_videos(max_dist)
            records = np.zeros(cross.size + among.size, dtype=VMATCH_DTYPE)
            head, tail = records[:cross.size], records[cross.size:]
            head["a"], head["b"], head["q_hits"], head["t_hits"] = cross["b"], cross["a"] + VT, cross["t_hits"], cross["q_hits"]
            tail["a"], tail["b"], tail["q_hits"], tail["t_hits"] = among["a"] + VT, among["b"] + VT, among["q_hits"], among["t_hits"]
            records = records[np.lexsort((records["b"], records["a"]))]
        return Ingest(union, records, dropped)

    def free(self) -> None:
        for b in (self.d_hashes, self.d_offsets, self.d_video, self.d_img, self.d_positions, self.d_spread, self.d_weights):
            if b is not None:
                b.free()
        self.d_weights = None
        self.d_img = None
        self.d_positions = None
        self.d_spread = None
        self.spread_max_dist = None


class DeviceQueries(DeviceLibrary):
    """The query operand of the transformed search (DeviceLibrary.from_raw_dihedral): the kept frames of every video v
    under each of the K non-identity transforms, query video v*K + k for transforms[k], d_excl = v per frame."""

    def __init__(self, d_hashes: DeviceBuffer, d_video: DeviceBuffer, d_excl: DeviceBuffer, n_frames: int, n_videos: int,
                 transforms: tuple):
        super().__init__(d_hashes, None, d_video, n_frames, n_videos)
        self.d_excl, self.transforms = d_excl, transforms

    def offsets(self) -> np.ndarray:
        raise NotImplementedError("a query set has no CSR of its own: query video v*K + k has video v's kept frames")

    def free(self) -> None:
        super().free()
        self.d_excl.free()


def _search_records(launch, cap: int) -> np.ndarray:
    """One device video search: launch(d_out, cap, d_count) -> status, then the records sorted by (a, b)."""
    lib = _lib.ensure()
    # the record buffer is kept from call to call (per context): two hipMalloc / hipFree round trips inside every search were
    # ~1 % of a 50 000-video pass during which the GPU did nothing. Buffer, launch and read-back stay under the context's
    # lock: two threads searching on one context would otherwise read each other's records, or free a buffer the other
    # is still reading back.
    with _record_lock():
        d_out, d_cnt, _ = _record_buffers(cap)  # (the call is told `cap` as asked, whatever the kept buffer would hold)
        _lib.check(launch(d_out.ptr, cap, d_cnt.ptr))
        cnt = int(d_cnt.to_array(np.uint64, 1)[0])
        if cnt > cap:  # more video pairs than room: ONLY the emit is repeated (no second O(n^2) pass, no second
            # key exchange that every rank would have to enter in lock-step)
            cap = cnt
            d_out, d_cnt, _ = _record_buffers(cap)
            _lib.check(lib.hvd_dev_vpdq_emit_again(d_out.ptr, cap, d_cnt.ptr))
            cnt = int(d_cnt.to_array(np.uint64, 1)[0])
            assert cnt <= cap
        recs = d_out.to_array(VMATCH_DTYPE, cnt)
    # ((a, b) is unique, so the sort need not be stable: numpy's default 64-bit sort is three times faster on 21 k records)
    return recs[np.argsort((recs["a"].astype(np.uint64) << np.uint64(32)) | recs["b"])]


_RECORD_BUFFERS: dict = {}  # context index -> (d_out, d_cnt, cap): grow-only, released by release_record_buffers()
_RECORD_LOCKS: dict = {}    # context index -> lock held from the buffer lookup to the end of the read-back
_RECORD_MU = threading.Lock()


def _record_lock():
    ctx = _lib.load().hvd_get_context()
    with _RECORD_MU:
        lk = _RECORD_LOCKS.get(ctx)
        if lk is None:
            lk = _RECORD_LOCKS[ctx] = threading.Lock()
    return lk



def _record_buffers(cap: int):
    """(caller holds _record_lock())"""
    ctx = _lib.load().hvd_get_context()
    have = _RECORD_BUFFERS.get(ctx)
    if have is None or have[2] < cap or have[0].ptr is None:
        if have is not None:
            have[0].free()
            have[1].free()
        have = (DeviceBuffer(16 * cap), DeviceBuffer(8), cap)
        with _RECORD_MU:
            _RECORD_BUFFERS[ctx] = have
    return have


def release_record_buffers() -> None:
    with _RECORD_MU:
        for d_out, d_cnt, _ in _RECORD_BUFFERS.values():
            d_out.free()
            d_cnt.free()
        _RECORD_BUFFERS.clear()


def shard_frames(raw_offsets: np.ndarray, world: int) -> int:
    """Frames in the longest rank's share (shards are padded to it for the equal-size all-gather)."""
    V = raw_offsets.size - 1
    ranges = (video_range_of_rank(V, r, world) for r in range(world))
    return max(int(raw_offsets[hi] - raw_offsets[lo]) for lo, hi in ranges)


def gather_hash_shards(d_h: DeviceBuffer, d_q: DeviceBuffer, raw_offsets: np.ndarray, rank: int, world: int, exchange,
                       hash_bytes: int = 32):
    """All-gather of the per-rank hash / quality shards (RCCL, equal-size padded blocks), then the padding is
    squeezed out so that the frames are in library order. hash_bytes: per frame (256 for the dihedral hashes).
    -> (d_hashes, d_quality) for the whole library."""
    lib = _lib.ensure()
    V = raw_offsets.size - 1
    n_total = int(raw_offsets[-1])
    v_lo, v_hi = video_range_of_rank(V, rank, world)
    n_mine = int(raw_offsets[v_hi] - raw_offsets[v_lo])
    shard = max(1, shard_frames(raw_offsets, world))
    with _DeviceScope() as scope:
        d_all_h, d_all_q = scope.temp(DeviceBuffer(hash_bytes * shard * world)), scope.temp(DeviceBuffer(4 * shard * world))
        d_ph, d_pq = scope.temp(DeviceBuffer(hash_bytes * shard)), scope.temp(DeviceBuffer(4 * shard))  # my shard, padded
        d_ph.zero()
        d_pq.zero()
        _lib.check(lib.hvd_memcpy_d2d(d_ph.ptr, d_h.ptr, hash_bytes * n_mine))
        _lib.check(lib.hvd_memcpy_d2d(d_pq.ptr, d_q.ptr, 4 * n_mine))
        exchange.allgather_bytes_dev(d_ph.ptr, d_all_h.ptr, hash_bytes * shard)
        exchange.allgather_bytes_dev(d_pq.ptr, d_all_q.ptr, 4 * shard)
        d_fh = scope.keep(DeviceBuffer(hash_bytes * max(n_total, 1)))
        d_fq = scope.keep(DeviceBuffer(4 * max(n_total, 1)))
        for r in range(world):  # ranks own contiguous video ranges
            lo, hi = video_range_of_rank(V, r, world)
            a, b = int(raw_offsets[lo]), int(raw_offsets[hi])
            if b > a:
                _lib.check(lib.hvd_memcpy_d2d(d_fh.ptr + hash_bytes * a, d_all_h.ptr + hash_bytes * shard * r,
                                              hash_bytes * (b - a)))
                _lib.check(lib.hvd_memcpy_d2d(d_fq.ptr + 4 * a, d_all_q.ptr + 4 * shard * r, 4 * (b - a)))
        _lib.check(lib.hvd_dev_sync())  # the staging buffers are freed on the way out
    return d_fh, d_fq


def _hashed_library(raw_offsets, rank: int, world: int, exchange, hash_stage, hash_bytes: int, compact, timings):
    """The front half of the chained entries, for one rank: this rank's videos are hashed, the hash shards all-gathered
    (world > 1), the whole library compacted, the raw hashes freed. The arguments are checked before any device work.
    hash_stage(mine) -> (d_hashes, d_quality) of this rank's frames, mine = the CSR of its videos counted from 0;
    hash_bytes: what it writes per frame; compact(d_hashes_ptr, d_quality_ptr, n, raw_offsets) -> returned as it is (a
    DeviceLibrary.from_raw_* constructor). timings (dict or None): receives gather_ms and compact_ms (host clock)."""
    raw_offsets = _check_raw_offsets(raw_offsets)
    if world > 1 and exchange is None:
        raise ValueError("world > 1 needs the RCCL exchange")
    v_lo, v_hi = video_range_of_rank(raw_offsets.size - 1, rank, world)
    d_h, d_q = hash_stage(raw_offsets[v_lo:v_hi + 1] - raw_offsets[v_lo])
    try:
        t0 = time.perf_counter()
        if world > 1:
            d_fh, d_fq = gather_hash_shards(d_h, d_q, raw_offsets, rank, world, exchange, hash_bytes)
            d_h.free()
            d_q.free()
            d_h, d_q = d_fh, d_fq
        t1 = time.perf_counter()
        out = compact(d_h.ptr, d_q.ptr, int(raw_offsets[-1]), raw_offsets)
        t2 = time.perf_counter()
    finally:
        d_h.free()
        d_q.free()
    if timings is not None:
        timings["gather_ms"] = (t1 - t0) * 1e3 if world > 1 else 0.0
        timings["compact_ms"] = (t2 - t1) * 1e3
    return out


def dedupe_frames_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                            threshold: float = 50.0, policy: str | None = None, rank: int = 0, world: int = 1,
                            exchange=None, keep_library: bool = False, timings: dict | None = None, autocrop=None):
    """BASELINE config 5 for one rank: the frames of videos [v_lo, v_hi) of this rank sit at d_frames_ptr
    (world == 1: all of them); raw_offsets is the CSR of the WHOLE library. Hash -> (all-gather of the hash
    shards) -> quality filter + CSR -> FP4 image -> sharded video search with the counters reduced on the GPU
    -> pair predicate of dedup.py:445-502 on the few video-level records.
    -> (pairs int64[m,2], records, library or None). Every rank returns the same result.
    timings (optional dict): receives hash_ms and search_ms, HIP-event times on the library stream of the hash launch
    and of the whole video search (image, probe, all-pairs pass, key reduction, record emit); gather_ms (host clock: the
    all-gather of the hash shards over RCCL incl. the squeeze into library order, 0 at world 1), compact_ms (host clock:
    quality filter + CSR, synchronous) and the search's own phases from the library (host clock, hvd_debug_get
    vmatch_us_*): search_local_ms (packed hashes, probe, all-pairs pass, key set), search_exchange_ms (agreement words,
    all-gather of the key lists, merged set; 0 at world 1), search_fold_ms (keys -> pair map).
    autocrop (True, or a dict of black_level / min_bright): the hash stage becomes hvd_dev_content_rects +
    hvd_dev_pdq_hash_frames_rects over this rank's own videos (`hash_frames_autocrop_on_device`; a rank owns whole videos,
    so every rectangle sees all its frames); timings then also receives rects_ms. Everything after the hash stage is
    unchanged. A dict of bar_color / bar_level / min_bright (vpdq.autocrop_rule) finds the rectangles by the
    bar-colour rule instead; that form is for world == 1 (an array bar_color has one row per video of the library). A dict
    of detail (True) / detail_level / min_detail finds them by the detail rule, for world == 1 as well."""
    crop = vpdq.autocrop_rule(autocrop)
    if crop is not None and crop.kind == "detail" and world != 1:
        raise ValueError("the detail rule is not sharded over a device group: world must be 1")
    if crop is not None and crop.kind == "color" and world != 1:
        raise ValueError("the bar-colour rule is not sharded over a device group: world must be 1")
    timed = _stage_timer(timings)

    def hash_stage(mine):
        n_mine = int(mine[-1])
        if crop is None:
            return timed("hash_ms", lambda: hash_frames_on_device(d_frames_ptr, n_mine, h, w, channels))
        d_h, d_q, d_r = hash_frames_autocrop_on_device(d_frames_ptr, n_mine, h, w, channels, mine, timed=timed, **crop.kwargs())
        d_r.free()
        return d_h, d_q

    library = _hashed_library(raw_offsets, rank, world, exchange, hash_stage, 32, DeviceLibrary.from_raw_hashes, timings)
    recs = timed("search_ms", lambda: library.match_videos(rank=rank, world=world))
    if timings is not None:
        lib = _lib.ensure()
        us = C.c_int(0)
        for key in ("local", "exchange", "fold"):
            _lib.check(lib.hvd_debug_get(f"vmatch_us_{key}".encode(), C.byref(us)))
            timings[f"search_{key}_ms"] = us.value / 1e3
    pairs = search.similar_video_pairs(recs, library.lengths(), threshold, policy)
    if keep_library:
        return pairs, recs, library
    library.free()
    return pairs, recs, None


def dedupe_frames_without_common_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                           max_videos: int, max_share: int = 50, threshold: float = 50.0,
                                           policy: str | None = None, min_quality: int = vpdq.QUALITY_TOLERANCE):
    """`dedupe_frames_on_device` with the common-frame filter between the quality filter and the search, on
    the calling thread's context: hash -> quality filter + CSR -> spread -> rule -> compaction -> the video search on what
    is left -> pair predicate. max_videos / max_share: DeviceLibrary.without_common_frames. -> (pairs int64[m,2], records,
    dropped int64[V], timings); the records' counters and the predicate's lengths are those of the filtered library.
    timings: hash_ms, common_ms (spread, rule, compaction) and search_ms, HIP-event times on the library stream;
    compact_ms (host clock: quality filter + CSR, synchronous)."""
    search.check_common_rule(max_videos, max_share)
    timings: dict = {}
    timed = _stage_timer(timings)
    library = _hashed_library(
        raw_offsets, 0, 1, None, lambda mine: timed("hash_ms", lambda: hash_frames_on_device(d_frames_ptr, int(mine[-1]), h, w, channels)),
        32, lambda d_h, d_q, n, raw: DeviceLibrary.from_raw_hashes(d_h, d_q, n, raw, min_quality), timings)
    del timings["gather_ms"]
    try:
        filtered, dropped = timed("common_ms", lambda: library.without_common_frames(max_videos, max_share))
    finally:
        library.free()
    try:
        recs = timed("search_ms", filtered.match_videos)
        pairs = search.similar_video_pairs(recs, filtered.lengths(), threshold, policy)
    finally:
        filtered.free()
    return pairs, recs, dropped, timings


def dedupe_frames_without_repeats_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                            max_dist: int, max_run: int = 0, threshold: float = 50.0,
                                            policy: str | None = None, min_quality: int = vpdq.QUALITY_TOLERANCE,
                                            weighted: bool = False, max_weight: int = 0):
    """`dedupe_frames_on_device` with the static-scene filter between the quality filter and the search, on the
    calling thread's context: hash -> quality filter + CSR -> runs of near-identical frames -> compaction -> the video search
    on what is left -> pair predicate. max_dist / max_run: DeviceLibrary.without_repeated_frames. -> (pairs int64[m,2],
    records, dropped int64[V], timings); the records' counters and the predicate's lengths are those of the collapsed library.
    timings: hash_ms, runs_ms (rule, compaction, gathers) and search_ms, HIP-event times on the library stream; compact_ms
    (host clock: quality filter + CSR, synchronous).
    weighted=True: the runs become the collapsed library's weights, the search is the weighted one, and the
    predicate's lengths are `weight_totals(max_weight)` -- a kept frame counts for min(run, max_weight) frames (max_weight 0:
    for its run; at max_dist 0 the records are then those of the library before the collapse). The totals' time is part of
    search_ms."""
    search.check_run_rule(max_dist, max_run)
    if int(max_weight) != max_weight or max_weight < 0 or (max_weight and not weighted):
        raise ValueError("max_weight is an integer, at least 0 (0 = no cap), and needs weighted=True")
    timings: dict = {}
    timed = _stage_timer(timings)
    library = _hashed_library(
        raw_offsets, 0, 1, None, lambda mine: timed("hash_ms", lambda: hash_frames_on_device(d_frames_ptr, int(mine[-1]), h, w, channels)),
        32, lambda d_h, d_q, n, raw: DeviceLibrary.from_raw_hashes(d_h, d_q, n, raw, min_quality), timings)
    del timings["gather_ms"]
    try:
        collapsed, dropped, d_runs = timed("runs_ms", lambda: library.without_repeated_frames(max_dist, max_run))
        if weighted:
            collapsed.attach_weights(d_runs)
        else:
            d_runs.free()
    finally:
        library.free()
    try:
        if weighted:
            recs, lengths = timed("search_ms", lambda: (collapsed.match_videos(weighted=True, max_weight=max_weight),
                                                         collapsed.weight_totals(max_weight)))
        else:
            recs, lengths = timed("search_ms", collapsed.match_videos), collapsed.lengths()
        pairs = search.similar_video_pairs(recs, lengths, threshold, policy)
    finally:
        collapsed.free()
    return pairs, recs, dropped, timings


def _groups_on_device(grouping, d_records_ptr, n_records, d_record_count_ptr, kind, d_lengths_ptr, T, is_min, V, d_score_ptr,
                      accept=None):
    """The device entry of `grouping` (search.COMPONENTS or search.KEEPER_FIRST) over records that lie in HBM, behind
    group_records_on_device and keeper_groups_on_device -> (node array, groups, rounds), or None when accept() refused; rounds
    stays 0 where the entry reports none."""
    lib = _lib.ensure()
    sb = C.c_size_t(0)
    _lib.check(getattr(lib, grouping.scratch_entry)(V, C.byref(sb)))
    cap = max(1, min(V // 2, n_records))  # a group has two members and one record at least
    rounds = C.c_int64(0)
    with _DeviceScope() as scope:
        d_scr, d_node = scope.temp(DeviceBuffer(sb.value)), scope.temp(DeviceBuffer(4 * V))
        d_groups, d_cnt = scope.temp(DeviceBuffer(16 * cap)), scope.temp(DeviceBuffer(8))
        _lib.check(getattr(lib, grouping.device_entry)(
            d_records_ptr, n_records, d_record_count_ptr, kind, d_lengths_ptr, T, int(is_min), V, d_score_ptr, d_scr.ptr, d_node.ptr,
            d_groups.ptr, cap, d_cnt.ptr, *((C.byref(rounds),) if grouping.rounds else ())))
        out = None
        if accept is None or accept():
            count = int(d_cnt.to_array(np.uint64, 1)[0])  # (the copy waits for the library stream)
            assert count <= cap
            out = d_node.to_array(np.int32, V), d_groups.to_array(GROUP_DTYPE, count), rounds.value
        _lib.check(lib.hvd_dev_sync())  # nothing may still run on a buffer that is freed here
    return out


def group_records_on_device(d_records_ptr: int, n_records: int, d_record_count_ptr, V: int, d_score_ptr=None,
                            accept=None) -> tuple[np.ndarray, np.ndarray] | None:
    """hvd_dev_group_edges (HVD_EDGES_ALL) over records that lie in HBM -> (labels, groups) as search.group_edges returns them;
    only those cross PCIe. d_record_count_ptr: None, or the uint64 an all-pairs entry counted its records in: the grouping is
    then enqueued behind that pass with no read-back in between and takes min(count, n_records) records. accept(): called after
    the launches and before anything is downloaded; returning False drops the result (-> None)."""
    out = _groups_on_device(search.COMPONENTS, d_records_ptr, n_records, d_record_count_ptr, _lib.EDGES_ALL, None, 0, False, V,
                            d_score_ptr, accept)
    return None if out is None else out[:2]


def cluster_hashes_on_device(d_db_ptr: int, n: int, max_dist: int = search.DISTANCE_TOLERANCE, pair_cap: int | None = None,
                             score=None, variant: int = search.DEFAULT_VARIANT) -> tuple[np.ndarray, np.ndarray]:
    """Groups of near-duplicate hashes with the pair list never leaving HBM: n packed hashes at d_db_ptr -> FP4 image ->
    hvd_dev_allpairs_hamming256_mfma (every i < j within max_dist, appended to a pair buffer of pair_cap records) ->
    hvd_dev_group_edges over that buffer and its device-side count, enqueued without a read-back -> (labels, groups) as
    search.group_edges(search.allpairs_hamming(db, max_dist), n) returns them. The one number read before the download is the
    pair count: when it exceeded the buffer, the pass is repeated with a buffer of exactly that size (the spirit of
    _lib.records_with_retry). score: uint32 per hash for the keeper, default all 0 (the smallest index)."""
    lib = _lib.ensure()
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=GROUP_DTYPE)
    score = search._score_array(score, n)
    cap = max(4096, 8 * n) if pair_cap is None else max(1, int(pair_cap))
    sz = C.c_size_t(0)
    _lib.check(lib.hvd_fp4_image_bytes(n, C.byref(sz)))
    with _DeviceScope() as scope:
        d_img = scope.temp(DeviceBuffer(sz.value))
        d_score = scope.temp(DeviceBuffer.from_array(score) if score is not None else None)
        d_cnt = scope.temp(DeviceBuffer(8))
        _lib.check(lib.hvd_dev_expand_fp4(d_db_ptr, n, d_img.ptr))
        found = 0

        def pairs_fit():
            nonlocal found
            found = int(d_cnt.to_array(np.uint64, 1)[0])  # (the copy waits for the library stream)
            return found <= cap

        while True:
            d_pairs = scope.temp(DeviceBuffer(16 * cap))
            d_cnt.zero()
            _lib.check(lib.hvd_dev_allpairs_hamming256_mfma(d_db_ptr, d_img.ptr, n, None, int(max_dist), 0, 1, d_pairs.ptr, cap,
                                                            d_cnt.ptr, int(variant)))
            out = group_records_on_device(d_pairs.ptr, cap, d_cnt.ptr, n, d_score.ptr if d_score else None, pairs_fit)
            if out is not None:
                return out
            d_pairs.free()  # (group_records_on_device has waited for the stream)
            cap = found


def _find_groups_on_device(grouping, d_frames_ptr, raw_offsets, h, w, channels, threshold, policy, score, keep_library):
    """The chain behind find_duplicate_groups_on_device and find_keeper_groups_on_device: `dedupe_frames_on_device`, the kept
    lengths, the grouping of its records, the fold -> (groups as the fold gives them, node array, group records, library or None)."""
    _, recs, library = dedupe_frames_on_device(d_frames_ptr, raw_offsets, h, w, channels, threshold, policy, keep_library=True)
    try:
        lengths = library.lengths()
        node, groups = search._grouped_records(grouping, recs, lengths, threshold, policy, lengths if score is None else score)
    except BaseException:
        library.free()
        raise
    if not keep_library:
        library.free()
        library = None
    return grouping.fold(node, groups), node, groups, library


def find_duplicate_groups_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                    threshold: float = 50.0, policy: str | None = None, score=None, keep_library: bool = False):
    """search.find_duplicate_groups on frames in HBM, one device: the chain of `dedupe_frames_on_device` (hash -> quality filter
    + CSR -> video search), then search.group_records over its records with the library's kept lengths: the pair predicate and
    the grouping run on the device. score: uint32 per video for the keeper; default the number of kept frames.
    -> (duplicate groups, labels, group records, library or None)."""
    return _find_groups_on_device(search.COMPONENTS, d_frames_ptr, raw_offsets, h, w, channels, threshold, policy, score, keep_library)


def keeper_groups_on_device(d_records_ptr: int, n_records: int, d_record_count_ptr, V: int, d_score_ptr=None,
                            kind: int = _lib.EDGES_ALL, d_lengths_ptr=None, T: int = 0, is_min: bool = False):
    """hvd_dev_keeper_groups over records that lie in HBM -> (keeper_of, groups, rounds): the first two as
    search.keeper_groups returns them, only those cross PCIe; rounds: how many rounds the keepers took. d_record_count_ptr as for
    `group_records_on_device`; the entry itself waits for the stream between its batches of rounds."""
    return _groups_on_device(search.KEEPER_FIRST, d_records_ptr, n_records, d_record_count_ptr, kind, d_lengths_ptr, T, is_min, V,
                             d_score_ptr)


def find_keeper_groups_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                 threshold: float = 50.0, policy: str | None = None, score=None, keep_library: bool = False):
    """search.find_keeper_groups on frames in HBM, one device: the chain of `dedupe_frames_on_device`, then
    search.keeper_group_records over its records with the library's kept lengths. score: uint32 per video, the larger is kept;
    default the number of kept frames. -> (keeper groups, keeper_of, group records, library or None)."""
    return _find_groups_on_device(search.KEEPER_FIRST, d_frames_ptr, raw_offsets, h, w, channels, threshold, policy, score, keep_library)


def _aligned_search_on_device(mode, d_frames_ptr, raw_offsets, h, w, channels, threshold, min_aligned, slack, positions, keep_library):
    """The chain of the excerpt searches on frames in HBM, one device: hash -> quality filter + CSR, with the kept frames' raw
    positions (`DeviceLibrary.from_raw_hashes(positions=True)`) -> video search -> the mode's alignment of its records -> the
    mode's fold (search.fold_aligned_records). -> (fold's result, search records, alignment records, library or None)."""
    library = _hashed_library(
        raw_offsets, 0, 1, None, lambda mine: hash_frames_on_device(d_frames_ptr, int(mine[-1]), h, w, channels), 32,
        lambda *raw: DeviceLibrary.from_raw_hashes(*raw, positions=bool(positions)), None)
    try:
        recs = library.match_videos()
        aligned = library._align(recs, mode, slack, None)
        lengths = library.lengths()
        out = search.fold_aligned_records(mode, aligned, lengths, search.similarity_of_records(recs, lengths), threshold, min_aligned)
    except BaseException:
        library.free()
        raise
    if keep_library:
        return out, recs, aligned, library
    library.free()
    return out, recs, aligned, None


def find_excerpts_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                            threshold: float = 50.0, min_aligned: int = 4, slack: int = search.ALIGN_SLACK,
                            positions: bool = True, keep_library: bool = False):
    """search.find_excerpts on frames in HBM, one device: hash -> quality filter + CSR, with the kept frames' raw positions
    (`DeviceLibrary.from_raw_hashes(positions=True)`) -> video search -> alignment of its records (`DeviceLibrary.align`) ->
    the keep rule of search.excerpts_from_records. raw_offsets: CSR of the videos over the frames at d_frames_ptr.
    positions=False aligns on the index inside the KEPT video instead: a frame the quality filter dropped then shifts
    everything after it (kept for comparison; the default is what a caller wants).
    -> (excerpts, search records, alignment records, library or None); Excerpt offsets / first / last are raw frame indices."""
    return _aligned_search_on_device(search.AlignMode(), d_frames_ptr, raw_offsets, h, w, channels, threshold, min_aligned, slack,
                                     positions, keep_library)


def find_segmented_excerpts_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                      threshold: float = 50.0, min_aligned: int = 4, slack: int = search.ALIGN_SLACK,
                                      positions: bool = True, max_segments: int = _lib.ALIGN_MAX_SEGMENTS,
                                      keep_library: bool = False):
    """search.find_segmented_excerpts on frames in HBM, one device: the chain of `find_excerpts_on_device` with the
    multi-segment alignment (`DeviceLibrary.align_segments`, min_band_votes = min_aligned) and the keep rule of
    search.segmented_excerpts_from_records; nothing but records crosses PCIe.
    -> (segmented excerpts, search records, VSEGMENTS records, library or None); positions are raw frame indices."""
    return _aligned_search_on_device(search.AlignMode(None, max_segments, int(min_aligned)), d_frames_ptr, raw_offsets, h, w,
                                     channels, threshold, min_aligned, slack, positions, keep_library)


def find_rate_excerpts_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                 threshold: float = 50.0, min_aligned: int = 4, slack: int = search.ALIGN_SLACK,
                                 rates=search.DEFAULT_RATES, positions: bool = True, keep_library: bool = False):
    """search.find_rate_excerpts on frames in HBM, one device: the chain of `find_excerpts_on_device` with the rate-aware
    alignment (`DeviceLibrary.align_rates`) and the keep rule of search.rate_excerpts_from_records; nothing but records
    crosses PCIe. -> (rate excerpts, search records, VRATE records, library or None); positions are raw frame indices."""
    return _aligned_search_on_device(search.AlignMode(rates), d_frames_ptr, raw_offsets, h, w, channels, threshold, min_aligned,
                                     slack, positions, keep_library)


def find_rate_segmented_excerpts_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                           threshold: float = 50.0, min_aligned: int = 4, slack: int = search.ALIGN_SLACK,
                                           rates=search.DEFAULT_RATES, positions: bool = True,
                                           max_segments: int = _lib.ALIGN_MAX_SEGMENTS, keep_library: bool = False):
    """search.find_rate_segmented_excerpts on frames in HBM, one device: the chain of `find_excerpts_on_device` with the
    rate-aware multi-segment alignment (`DeviceLibrary.align_rate_segments`, min_band_votes = min_aligned) and the keep rule of
    search.rate_segmented_excerpts_from_records; nothing but records crosses PCIe.
    -> (rate-segmented excerpts, search records, VRSEGMENTS records, library or None); positions are raw frame indices."""
    return _aligned_search_on_device(search.AlignMode(rates, max_segments, int(min_aligned)), d_frames_ptr, raw_offsets, h, w,
                                     channels, threshold, min_aligned, slack, positions, keep_library)


def find_reversed_excerpts_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                     threshold: float = 50.0, min_aligned: int = 4, slack: int = search.ALIGN_SLACK,
                                     rates=search.REVERSED_RATES, positions: bool = True,
                                     max_segments: int = _lib.ALIGN_MAX_SEGMENTS, keep_library: bool = False):
    """search.find_reversed_excerpts on frames in HBM, one device: the chain of `find_excerpts_on_device` with the alignment
    with negative rates (`DeviceLibrary.align_signed`, min_band_votes = min_aligned) and the keep rule of
    search.signed_excerpts_from_records; nothing but records crosses PCIe.
    -> (rate-segmented excerpts, search records, VSSEGMENTS records, library or None); positions are raw frame indices."""
    return _aligned_search_on_device(search.AlignMode(rates, max_segments, int(min_aligned), True), d_frames_ptr, raw_offsets, h, w,
                                     channels, threshold, min_aligned, slack, positions, keep_library)


def find_looped_excerpts_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                   threshold: float = 50.0, min_aligned: int = 4, rates=search.REVERSED_RATES,
                                   max_rounds: int = _lib.ALIGN_MAX_ROUNDS, slack: int = search.ALIGN_SLACK, positions: bool = True,
                                   keep_library: bool = False):
    """search.find_looped_excerpts on frames in HBM, one device: the chain of `find_excerpts_on_device` up to the video search,
    then every record aligned in both orientations, (a, b) and then (b, a), in one `DeviceLibrary.align_loops` call
    (min_band_votes = min_aligned), and the keep rule of search.looped_excerpts_from_records; nothing but records crosses PCIe.
    -> (looped excerpts, search records, VLOOPS records -- twice as many --, library or None); positions are raw frame indices."""
    library = _hashed_library(
        raw_offsets, 0, 1, None, lambda mine: hash_frames_on_device(d_frames_ptr, int(mine[-1]), h, w, channels), 32,
        lambda *raw: DeviceLibrary.from_raw_hashes(*raw, positions=bool(positions)), None)
    try:
        recs = library.match_videos()
        ab = np.stack([recs["a"], recs["b"]], axis=1)
        aligned = library.align_loops(np.concatenate([ab, ab[:, ::-1]]), rates, slack, None, max_rounds, int(min_aligned))
        lengths = library.lengths()
        out = search.looped_excerpts_from_records(aligned, lengths, np.tile(search.similarity_of_records(recs, lengths), 2), threshold)
    except BaseException:
        library.free()
        raise
    if keep_library:
        return out, recs, aligned, library
    library.free()
    return out, recs, aligned, None


def find_compilations_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                threshold: float = 50.0, min_aligned: int = 4, slack: int = search.ALIGN_SLACK,
                                positions: bool = True, keep_library: bool = False):
    """search.find_compilations on frames in HBM, one device: hash -> quality filter + CSR, with the kept frames' raw positions
    -> video search -> alignment of its records with the union of every video's aligned frames (`DeviceLibrary.cover`) -> the
    keep rule of search.compilations_from_records; nothing but records crosses PCIe. The arguments are
    `find_excerpts_on_device`'s. -> (compilations, search records, alignment records, cover records, library or None);
    first / last / offset of a source are raw frame indices."""
    library = _hashed_library(
        raw_offsets, 0, 1, None, lambda mine: hash_frames_on_device(d_frames_ptr, int(mine[-1]), h, w, channels), 32,
        lambda *raw: DeviceLibrary.from_raw_hashes(*raw, positions=bool(positions)), None)
    try:
        recs = library.match_videos()
        aligned, cover = library.cover(recs, slack, None, min_aligned)
        out = search.compilations_from_records(aligned, cover, library.lengths(), threshold, min_aligned)
    except BaseException:
        library.free()
        raise
    if keep_library:
        return out, recs, aligned, cover, library
    library.free()
    return out, recs, aligned, cover, None


def _rank0_of_every_context(entry, frames_of_rank, timings, n_results: int, *args, **kwargs):
    """entry(frames_of_rank(rank, world), *args, rank, world, exchange, timings, **kwargs) on one thread per context of the
    in-process device group, rank = context index. -> the first n_results values rank 0 returned (every rank computes the
    same); timings receives rank 0's stage times."""
    from . import multigpu

    def one(rank, world):
        ex = multigpu.GroupExchange(rank, world) if world > 1 else None
        tm = {} if timings is not None and rank == 0 else None
        out = entry(frames_of_rank(rank, world), *args, rank=rank, world=world, exchange=ex, timings=tm, **kwargs)
        if tm is not None:
            timings.update(tm)
        return out[:n_results]

    return multigpu.run_on_contexts(one)[0]


def dedupe_frames_in_process(frames_of_rank, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                             threshold: float = 50.0, policy: str | None = None, timings: dict | None = None, autocrop=None):
    """BASELINE config 5 on the library's in-process device group (hvd_init_devices / HVD_DEVICES), no launcher:
    one thread per context runs `dedupe_frames_on_device` as rank = context index. frames_of_rank(rank, world) ->
    device pointer of the frames of that rank's video range (`video_range_of_rank`), resident on that rank's device (it is
    called on the rank's thread, with the rank's context current). -> (pairs, records) -- every rank computes the same;
    rank 0's are returned. timings: rank 0's stage times. autocrop: as `dedupe_frames_on_device`."""
    # a bad value fails here, not on every rank's thread; a group takes the black rule only
    rule = vpdq.autocrop_rule(autocrop)
    if rule is not None and rule.kind == "detail":
        raise ValueError("the detail rule is not sharded over a device group: world must be 1 (dedupe_frames_on_device)")
    if rule is not None and rule.kind == "color":
        vpdq.autocrop_params(rule.kwargs())  # raises: the black rule's keys only
    return _rank0_of_every_context(dedupe_frames_on_device, frames_of_rank, timings, 2, raw_offsets, h, w, channels,
                                   threshold, policy, autocrop=autocrop)


def dedupe_transformed_frames_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                        threshold: float = 50.0, policy: str | None = None, transforms="mirror",
                                        rank: int = 0, world: int = 1, exchange=None, keep_library: bool = False,
                                        timings: dict | None = None):
    """`dedupe_frames_on_device` that also finds mirrored / flipped / rotated copies (search.find_transformed_duplicates
    on frames in HBM). Dihedral hash -> (all-gather of the 256 B/frame shards) -> quality filter + CSR of the identity
    library and of the query set of the other selected variants (hvd_dev_compact_kept_dihedral) -> FP4 images -> video
    search of the identity library -> one cross search of the query set against it -> search.fold_transformed_records.
    transforms: what search.transform_set takes ("mirror", "flips", "dihedral" or names including "identity").
    -> (pairs int64[m,2], transform int64[m] (vpdq.TRANSFORMS index), similarity float64[m], identity records, cross
    records, identity library or None). Every rank returns the same result. timings (optional dict): hash_ms, search_ms
    and cross_ms (HIP events on the library stream), gather_ms and compact_ms (host clock, as in dedupe_frames_on_device)."""
    names = search.transform_set(transforms)
    cross = [t for t in names if t != "identity"]
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    timed = _stage_timer(timings)
    library, queries = _hashed_library(
        raw_offsets, rank, world, exchange,
        lambda mine: timed("hash_ms", lambda: hash_frames_dihedral_on_device(d_frames_ptr, int(mine[-1]), h, w, channels)), 256,
        lambda *raw: DeviceLibrary.from_raw_dihedral(*raw, names), timings)
    try:
        # the identity records are read back before the cross search: emit-again state belongs to the last search only
        recs_i = timed("search_ms", lambda: library.match_videos(rank=rank, world=world))
        recs_c = timed("cross_ms", lambda: library.match_queries(queries, rank=rank, world=world)) if cross else \
            np.zeros(0, dtype=VMATCH_DTYPE)
    finally:
        if queries is not None:
            queries.free()
    if timings is not None:
        timings.setdefault("cross_ms", 0.0)
    pairs, tid, sim = search.fold_transformed_records(recs_i, recs_c, library.lengths(),
                                                      [vpdq.TRANSFORMS.index(t) for t in cross], threshold, policy,
                                                      return_similarity=True)
    if keep_library:
        return pairs, tid, sim, recs_i, recs_c, library
    library.free()
    return pairs, tid, sim, recs_i, recs_c, None


def dedupe_cropped_frames_on_device(d_frames_ptr: int, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                    threshold: float = 50.0, policy: str | None = None, crops="aspect",
                                    keep_library: bool = False, timings: dict | None = None):
    """`dedupe_frames_on_device` that also finds aspect-ratio re-crops of the listed centre crops
    (search.find_cropped_duplicates on frames in HBM; one device). Crop-ladder hash (the full frame and the K crops of every
    frame in one call) -> quality filter + CSR of the identity library and of the query set of the crop
    variants (hvd_dev_compact_kept_dihedral with the slot mask) -> FP4 images -> video search of the identity library ->
    one cross search of the query set against it -> search.fold_cropped_records. crops: what vpdq.crop_ladder takes.
    -> (duplicates: [search.CroppedDuplicate(a, b, crop, similarity, wide)], identity records, cross records, identity
    library or None). timings (optional dict): hash_ms, search_ms and cross_ms (HIP events on the library stream),
    gather_ms and compact_ms (host clock, as in dedupe_frames_on_device)."""
    names, _ = vpdq.crop_ladder(h, w, crops)  # a bad list fails here, before any device work
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    timed = _stage_timer(timings)

    def hash_stage(mine):
        d_h, d_q, _, _ = timed("hash_ms", lambda: hash_frames_crops_on_device(d_frames_ptr, int(mine[-1]), h, w, channels, crops,
                                                                                crop_quality=False))
        return d_h, d_q

    library, queries = _hashed_library(raw_offsets, 0, 1, None, hash_stage, 256,
                                       lambda *raw: DeviceLibrary.from_raw_crops(*raw, names), timings)
    try:
        try:
            # the identity records are read back before the cross search: emit-again state belongs to the last search only
            recs_i = timed("search_ms", lambda: library.match_videos())
            recs_c = timed("cross_ms", lambda: library.match_queries(queries))
        finally:
            if queries is not None:
                queries.free()
        folded = search.fold_cropped_records(recs_i, recs_c, library.lengths(), len(names), threshold, policy)
    except BaseException:
        library.free()
        raise
    dups = search.cropped_duplicates(*folded, names)
    if keep_library:
        return dups, recs_i, recs_c, library
    library.free()
    return dups, recs_i, recs_c, None


def dedupe_transformed_frames_in_process(frames_of_rank, raw_offsets: np.ndarray, h: int, w: int, channels: int,
                                         threshold: float = 50.0, policy: str | None = None, transforms="mirror",
                                         timings: dict | None = None):
    """`dedupe_frames_in_process` for `dedupe_transformed_frames_on_device`: one thread per context of the in-process
    device group, rank = context index, frames_of_rank(rank, world) as there. -> rank 0's (pairs, transform, similarity,
    identity records, cross records); every rank computes the same. timings: rank 0's stage times."""
    names = search.transform_set(transforms)  # a bad set fails here, not on every rank's thread
    return _rank0_of_every_context(dedupe_transformed_frames_on_device, frames_of_rank, timings, 5, raw_offsets, h, w,
                                   channels, threshold, policy, names)


def video_range_of_rank(V: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous share of the videos hashed by `rank` (frames are independent: no collective while hashing)."""
    per = (V + world - 1) // world
    lo = min(V, rank * per)
    return lo, min(V, lo + per)
