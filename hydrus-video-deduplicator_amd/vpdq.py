"""Drop-in for the native module ``hvdaccelerators.vpdq`` (PyPI hvdaccelerators==0.4.0),
i.e. exactly the five names the reference imports from it:

    vpdq.VideoHasher      vpdqpy/vpdqpy.py:113      VideoHasher(fps, w, h, num_threads)
      .hash_frame(bytes)  vpdqpy/vpdqpy.py:118
      .finish()->VpdqHash vpdqpy/vpdqpy.py:119
    vpdq.VpdqHash         vpdqpy/vpdqpy.py:25       .bytes (dedup.py:77), bytesPerPdqHash
                                                     (dedup.py:83), str() (hashing.py:30),
                                                     from_string (hashing.py:40), len/==/!=
                                                     (tests/unit_tests/test_vpdqpy.py:95,116)
    vpdq.matchHash        vpdqpy/vpdqpy.py:56       matchHash(q, t, tol) -> float in [0,100]
    vpdq.matchHashBytes   db/vptree.py:31           matchHashBytes(a, b, tol)

All arithmetic runs in HIP kernels on an MI355X through the C-ABI of
include/hvd_mi355x.h; there is no CPU fallback.

Semantics that the (absent) wheel does not let us pin are explicit, tested policies
(SURVEY.md 3.5), each selectable by an environment variable or at run time:

* ``MATCH_COMPARATOR`` (``HVD_MATCH_COMPARATOR`` = ``le`` | ``lt``): a frame pair is a hit when
  ``hamming <= tolerance`` (default) or ``hamming < tolerance``. Distances are integers, so ``lt``
  is ``le`` at ``tolerance - 1``; the kernels always take the inclusive bound (``frame_max_dist``).
  UNVERIFIED DEFAULT: upstream's matchTwoHashBrute may be strict; tests/golden/import_reference.py
  settles it where the wheel is installable.
* ``MATCH_POLICY`` (``HVD_MATCH_POLICY``): reduction of the two vPDQ percentages (query-matched %,
  target-matched %) to one number; default "min", the only symmetric choice, which
  dedup.py:502's ``// 2`` assumes.
"""

from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import NamedTuple

import numpy as np

from . import _lib

BYTES_PER_PDQ_HASH = 32
QUALITY_TOLERANCE = 31  # frames with quality >= 31 are kept (db/DedupeDB.py:550-553)

# "min" | "max" | "query" | "target"; see module docstring.
MATCH_POLICY = os.environ.get("HVD_MATCH_POLICY", "min")
_POLICIES = ("min", "max", "query", "target")

# "le" | "lt"; see module docstring.
MATCH_COMPARATOR = os.environ.get("HVD_MATCH_COMPARATOR", "le")
_COMPARATORS = ("le", "lt")


def policy_labels() -> dict:
    """The semantic switches the absent `hvdaccelerators` wheel leaves open, as labels for every artefact that reports
    results (bench.py's JSON line, hvd_runtime_info): `(unverified)` marks a DEFAULT that nothing reference-held confirms;
    a value set explicitly through the environment is the caller's decision and carries no mark."""
    return {"comparator": MATCH_COMPARATOR + ("" if "HVD_MATCH_COMPARATOR" in os.environ else " (unverified)"),
            "reduction": MATCH_POLICY + ("" if "HVD_MATCH_POLICY" in os.environ else " (unverified)"),
            "dct": "strict" if _lib_dct_mode() == 0 else "fma",
            "hash_text": "hex, 64 characters per frame (unverified)"}


def _lib_dct_mode() -> int:
    try:
        return int(_lib.load().hvd_get_pdq_dct_mode())
    except Exception:  # noqa: BLE001 - labels must be printable without the library
        return 0 if os.environ.get("HVD_PDQ_DCT_MODE", "strict") != "fma" else 1


_warned_unverified = False


def warn_unverified_policies() -> None:
    """One RuntimeWarning per process, the first time a matchHash* entry runs with the comparator left at its unverified
    default: upstream's matchTwoHashBrute may compare with a strict `<`."""
    global _warned_unverified
    if _warned_unverified or "HVD_MATCH_COMPARATOR" in os.environ:
        return
    _warned_unverified = True
    import warnings

    warnings.warn("hvd_amd: frame comparator left at its default 'le' (a frame pair at Hamming distance == tolerance is a hit); "
                  "hvdaccelerators 0.4.0 could not be consulted and upstream vPDQ may use a strict '<'. Set "
                  "HVD_MATCH_COMPARATOR=le|lt to state the choice (INTEGRATION.md section 4).", RuntimeWarning, stacklevel=3)


def frame_max_dist(distance_tolerance, comparator: str | None = None) -> int:
    """Inclusive Hamming bound the kernels use for a reference-style tolerance under the comparator
    policy: tolerance for "le", tolerance - 1 for "lt" (-1 = nothing matches)."""
    comparator = MATCH_COMPARATOR if comparator is None else comparator
    if comparator not in _COMPARATORS:
        raise ValueError(f"unknown comparator {comparator!r}; expected one of {_COMPARATORS}")
    tol = int(distance_tolerance)
    return tol if comparator == "le" else tol - 1


def set_dct_mode(mode: str) -> None:
    """"strict" (default): separately rounded multiply and add, the numerics of upstream's x86-64
    builds; "fma": fused multiply-add on the matrix cores, the numerics of upstream's arm64 builds
    (opt-in; ~2 % of hash bits differ between the two). See include/hvd_mi355x.h."""
    modes = {"strict": 0, "fma": 1}
    if mode not in modes:
        raise ValueError(f"unknown DCT mode {mode!r}; expected one of {sorted(modes)}")
    _lib.check(_lib.load().hvd_set_pdq_dct_mode(modes[mode]))


def get_dct_mode() -> str:
    return ("strict", "fma")[_lib.load().hvd_get_pdq_dct_mode()]


def percent_from_hits(q_hits: int, t_hits: int, nq: int, nt: int, policy: str | None = None) -> float:
    """vPDQ match percentage from the kernel's two counters (either side empty -> 0.0,
    db/DedupeDB.py:555-557)."""
    policy = MATCH_POLICY if policy is None else policy
    if policy not in _POLICIES:
        raise ValueError(f"unknown match policy {policy!r}; expected one of {_POLICIES}")
    if nq <= 0 or nt <= 0:
        return 0.0
    qp = (q_hits * 100.0) / nq
    tp = (t_hits * 100.0) / nt
    if policy == "min":
        return min(qp, tp)
    if policy == "max":
        return max(qp, tp)
    return qp if policy == "query" else tp


class VpdqHash:
    """Immutable value: N concatenated 32-byte PDQ frame hashes (N >= 0)."""

    bytesPerPdqHash = BYTES_PER_PDQ_HASH
    __slots__ = ("_b",)

    def __init__(self, data: bytes = b""):
        data = bytes(data)
        if len(data) % BYTES_PER_PDQ_HASH != 0:
            raise ValueError(f"VpdqHash needs a multiple of {BYTES_PER_PDQ_HASH} bytes, got {len(data)}")
        self._b = data

    @property
    def bytes(self) -> bytes:
        return self._b

    def __len__(self) -> int:
        return len(self._b) // BYTES_PER_PDQ_HASH

    def __eq__(self, other) -> bool:
        return isinstance(other, VpdqHash) and self._b == other._b

    def __ne__(self, other) -> bool:
        return not self.__eq__(other)

    def __hash__(self) -> int:
        return hash(self._b)

    def __str__(self) -> str:
        # contiguous lowercase hex of .bytes, 64 chars per frame, single line
        # (db/DedupeDB.py:547-559; tests read it back with readline(), test_benchmark_vpdqpy.py:58-59)
        return self._b.hex()

    def __repr__(self) -> str:
        return f"VpdqHash(frames={len(self)})"

    @staticmethod
    def from_string(s: str) -> "VpdqHash":
        s = s.strip()
        if len(s) % (2 * BYTES_PER_PDQ_HASH) != 0:
            raise ValueError("VpdqHash string must be 64 hex characters per frame")
        try:
            return VpdqHash(bytes.fromhex(s))
        except ValueError as exc:
            raise ValueError(f"invalid VpdqHash string: {exc}") from exc

    def frames(self) -> np.ndarray:
        """uint8[N,32] view of the frame hashes."""
        return np.frombuffer(self._b, dtype=np.uint8).reshape(-1, BYTES_PER_PDQ_HASH)


class VideoHasher:
    """Per-video frame hasher: the Python face of the native streaming hasher (hvd_hasher_*,
    csrc/hvd_stream.cpp). Frames are copied once into a ring of pinned batch slots; each batch is
    uploaded, hashed and downloaded on its own HIP stream, so PCIe transfer overlaps the PDQ
    kernels. ``hash_frame`` blocks only when every slot is still in flight, which bounds the
    staging memory like the reference's blocking frame queue (vpdqpy/vpdqpy.py:115-117). The
    reference's hasher runs a CPU thread pool instead; ``num_threads`` is accepted for signature
    compatibility; what it controls here is how many host threads share the copy of one frame into the ring
    (0 = library default). One hasher per decoder thread.

    ``transforms``: None (default) is the plain hasher. A set name of ``search.transform_set`` ("mirror", "flips",
    "dihedral") or a sequence of ``TRANSFORMS`` names makes it a dihedral hasher (hvd_hasher_create_dihedral): the same
    ring, every batch hashed by the dihedral kernel. ``finish_transformed()`` then returns ``{name: VpdqHash}`` for those
    names and ``finish()`` the identity hash, which is what the plain hasher returns. Strict DCT mode only: in the "fma"
    mode the constructor raises HvdError.

    ``autocrop``: None (default) hashes whole frames. True, or a dict with ``black_level`` / ``min_bright`` (what
    ``autocrop_params`` takes), makes it an autocrop hasher (hvd_hasher_create_autocrop): the video's frames
    stay in device memory while they stream in, their content rectangle is folded batch by batch behind the uploads, and
    ``finish()`` hashes every frame inside that rectangle -- the result of ``hash_frames_autocrop`` on the same frames as
    one video, byte for byte. After ``finish()``, ``rect`` is ``(top, left, height, width)``. ``max_retained_bytes``: how
    many bytes of frames one video may keep on the device (None: the library default, 8 GiB); the frame that would pass
    it raises HvdError(HVD_ERR_OVERFLOW) and ``finish()`` still returns the result of the frames taken before. Not
    together with ``transforms``. A dict with ``bar_color`` / ``bar_level`` raises a ValueError that names the
    array form (``hash_frames_autocrop(frames, bar_color=...)``): that colour is known only after the last frame.
    ``{"detail": True}``, with optional ``detail_level`` (default 8, unverified) / ``min_detail`` (default 8, unverified),
    is the detail rule (hvd_hasher_create_autocrop_detail): smooth bars of any colour -- blurred, gradient --
    are left out. It is order-free per frame, so it streams; ``finish()`` equals ``hash_frames_autocrop(frames, detail=True)``."""

    def __init__(self, average_fps: int, width: int, height: int, num_threads: int = 0,
                 batch_bytes: int = 32 << 20, transforms=None, autocrop=None, max_retained_bytes: int | None = None):
        if width < 64 or height < 64:
            raise ValueError("frames must be at least 64x64")
        if isinstance(autocrop, dict) and _KIND_KEYS["color"] & set(autocrop):
            raise ValueError("the streaming hasher has no bar-colour rule (the automatic colour is known only after the last "
                             "frame): hash the array form of the frames, vpdq.hash_frames_autocrop(frames, bar_color=...)")
        self._autocrop = autocrop_rule(autocrop)  # a RectRule of the black or the detail kind, or None
        if self._autocrop is not None and transforms is not None:
            raise ValueError("autocrop and transforms cannot be combined (content-rectangle dihedral hashing does not exist)")
        if max_retained_bytes is not None and (isinstance(max_retained_bytes, bool) or not isinstance(max_retained_bytes, (int, np.integer))
                                               or max_retained_bytes < 1):
            raise ValueError("max_retained_bytes must be a positive integer or None")
        self._max_retained = 0 if max_retained_bytes is None else int(max_retained_bytes)
        self.rect = None
        self._transforms = None
        if transforms is not None:
            from .search import transform_set

            self._transforms = transform_set(transforms, require_identity=False)
        self.average_fps = average_fps
        self.width = int(width)
        self.height = int(height)
        self.num_threads = num_threads
        self._frame_bytes_rgb = self.width * self.height * 3
        self._frame_bytes_gray = self.width * self.height
        self._batch_bytes = int(batch_bytes)
        self._channels = 0
        self._handle = None
        self._finished = False
        self._run = None        # acquire_frame(): view of the run of frames acquired from the native hasher ...
        self._run_pos = 0       # ... and how many of them commit_frame() has counted
        self._batch_run = None  # acquire_frames(): the run handed out
        self._lib = _lib.ensure()  # fail at construction, not at the first frame, if no GPU is usable
        if self._transforms is not None and self._lib.hvd_get_pdq_dct_mode() != 0:
            # the native hasher is created at the first frame (its pixel format decides the channels): fail here instead
            raise _lib.HvdError(_lib.HVD_ERR_STATE, "dihedral hashing has no fma DCT mode: set_dct_mode('strict') first")

    def _open(self, channels: int) -> None:
        frame_bytes = self._frame_bytes_rgb if channels == 3 else self._frame_bytes_gray
        batch = max(1, min(4096, self._batch_bytes // frame_bytes))
        h = C.c_void_p()
        if self._autocrop is not None:
            create = getattr(self._lib, "hvd_hasher_create_autocrop" + _RECT_KINDS[self._autocrop.kind].dev)
            _lib.check(create(self.width, self.height, channels, batch, self._autocrop.level, self._autocrop.count,
                              self._max_retained, C.byref(h)))
        else:
            create = self._lib.hvd_hasher_create if self._transforms is None else self._lib.hvd_hasher_create_dihedral
            _lib.check(create(self.width, self.height, channels, batch, C.byref(h)))
        self._handle = h
        self._channels = channels
        # num_threads: the reference hasher's worker threads (vpdqpy/vpdqpy.py:113; 0 = library default, negative =
        # "all but n cores", entrypoint.py:79-82) -> the threads that share the host-side copy of a frame into the ring
        nt = int(self.num_threads) if isinstance(self.num_threads, int) else 0
        if nt < 0:
            nt = max(1, (os.cpu_count() or 1) + nt)
        _lib.check(self._lib.hvd_hasher_set_threads(h, nt))

    def _check_feed(self, channels: int) -> None:
        if self._finished:
            raise RuntimeError("frame fed after finish()")
        if channels not in (1, 3):
            raise ValueError("channels must be 1 (gray) or 3 (rgb24)")
        if self._handle is None:
            self._open(channels)
        elif channels != self._channels:
            raise ValueError("all frames of one video must have the same pixel format")

    def _acquire_run(self, want: int) -> np.ndarray:
        """hvd_hasher_acquire_n: one view [got, h, w(, 3)] over the next `got` <= want frames of the pinned slot."""
        p, got = C.c_void_p(), C.c_int64(0)
        _lib.check(self._lib.hvd_hasher_acquire_n(self._handle, int(want), C.byref(p), C.byref(got)))
        ch = self._channels
        fb = self._frame_bytes_rgb if ch == 3 else self._frame_bytes_gray
        buf = (C.c_uint8 * (fb * got.value)).from_address(p.value)
        shape = (got.value, self.height, self.width, 3) if ch == 3 else (got.value, self.height, self.width)
        return np.frombuffer(buf, dtype=np.uint8).reshape(shape)

    def _flush_run(self) -> None:
        """Hand the frames committed one by one (commit_frame) to the native hasher: one hvd_hasher_commit_n per run."""
        if self._run is not None:
            n, self._run = self._run_pos, None
            self._run_pos = 0
            _lib.check(self._lib.hvd_hasher_commit_n(self._handle, n))

    def acquire_frames(self, k: int, channels: int = 3) -> np.ndarray:
        """Zero-copy feed for a RUN of frames (hvd_hasher_acquire_n): a writable uint8 view ``[got, height, width(, 3)]``
        of the pinned slot memory for the next frames, ``1 <= got <= k`` (what is left of the current batch slot, so a
        caller loops until its frames are placed); ``commit_frames(n)`` makes the first n count. One FFI round trip per
        run: a decoder of small frames (64x64) fills hundreds of frames per call. Blocks like ``hash_frame`` when every
        batch slot is in flight (vpdqpy/vpdqpy.py:115-117)."""
        if k < 1:
            raise ValueError("k must be at least 1")
        self._check_feed(channels)
        self._flush_run()
        self._batch_run = self._acquire_run(k)
        return self._batch_run

    def commit_frames(self, n: int | None = None) -> None:
        """The first n frames of the run ``acquire_frames`` handed out are complete (default: all of them)."""
        if self._batch_run is None:
            raise RuntimeError("commit_frames() without acquire_frames()")
        n = self._batch_run.shape[0] if n is None else int(n)
        self._batch_run = None
        _lib.check(self._lib.hvd_hasher_commit_n(self._handle, n))

    def acquire_frame(self, channels: int = 3) -> np.ndarray:
        """Zero-copy feed (hvd_hasher_acquire_n underneath): a writable uint8 view of the pinned slot memory for the NEXT
        frame -- shape (height, width, 3) or (height, width) -- so that a decoder can reformat straight into
        it (e.g. ``frame.to_ndarray(...)`` with ``out=``, or ``np.copyto``); ``commit_frame()`` makes it count.
        Blocks like ``hash_frame`` when every batch slot is in flight. The frames of one batch slot are handed out from ONE
        native call and committed with one (round 5: two ctypes calls and a buffer object per frame made this feed slower
        than ``hash_frame(bytes)`` for 64x64 frames)."""
        if self._run is None or self._run_pos == self._run.shape[0]:
            self._check_feed(channels)
            self._flush_run()
            self._run = self._acquire_run(1 << 30)  # the rest of the current batch slot
        elif channels != self._channels:
            raise ValueError("all frames of one video must have the same pixel format")
        return self._run[self._run_pos]

    def commit_frame(self) -> None:
        if self._run is None:
            raise RuntimeError("commit_frame() without acquire_frame()")
        self._run_pos += 1
        if self._run_pos == self._run.shape[0]:
            self._flush_run()  # the batch slot is full: submitted (H2D + kernels) by the native side

    def hash_frame(self, frame) -> None:
        """frame: packed RGB24 bytes (width*height*3, what bytes(frame.planes[0]) yields at
        vpdqpy.py:118) or gray bytes (width*height). The buffer is copied before returning."""
        if self._finished:
            raise RuntimeError("hash_frame() after finish()")
        if isinstance(frame, bytes):
            n, ptr, keep = len(frame), frame, frame
        else:
            keep = None
            if isinstance(frame, np.ndarray) and frame.flags.c_contiguous and frame.flags.writeable:
                # (0.3 us; `.ctypes.data` builds a helper object per call: 1.1 us of the 1 us a 64x64 frame costs otherwise)
                keep, n = frame, frame.nbytes
                ptr = C.addressof(C.c_uint8.from_buffer(frame))
            if keep is None:
                keep = np.frombuffer(frame, dtype=np.uint8)  # zero-copy view of any buffer object
                n, ptr = keep.size, keep.ctypes.data
        if n == self._frame_bytes_rgb:
            ch = 3
        elif n == self._frame_bytes_gray:
            ch = 1
        else:
            raise ValueError(f"frame has {n} bytes; expected {self._frame_bytes_rgb} (rgb24) or "
                             f"{self._frame_bytes_gray} (gray)")
        if self._handle is None:
            self._open(ch)
        elif ch != self._channels:
            raise ValueError("all frames of one video must have the same pixel format")
        if self._run is not None:
            self._flush_run()
        _lib.check(self._lib.hvd_hasher_push(self._handle, ptr))
        del keep

    def _drain(self) -> np.ndarray | None:
        """Ends the hasher: the hashes of the frames kept by the quality filter (>= QUALITY_TOLERANCE, once per frame),
        uint8[m,32] (plain) or uint8[m,8,32] (dihedral, TRANSFORMS order); None if no frame was fed."""
        self._finished = True
        if self._handle is None:
            if self._autocrop is not None:
                self.rect = (0, 0, self.height, self.width)
            return None
        try:
            self._flush_run()
            self._batch_run = None
            pending = C.c_int64(0)
            _lib.check(self._lib.hvd_hasher_pending(self._handle, C.byref(pending)))
            n = pending.value
            if self._transforms is None:
                shape, finish = (max(n, 1), BYTES_PER_PDQ_HASH), self._lib.hvd_hasher_finish
            else:
                shape, finish = (max(n, 1), len(TRANSFORMS), BYTES_PER_PDQ_HASH), self._lib.hvd_hasher_finish_dihedral
            hashes = np.zeros(shape, dtype=np.uint8)
            quality = np.zeros(max(n, 1), dtype=np.int32)
            got = C.c_int64(0)
            if self._autocrop is not None:
                rect = (C.c_int32 * 4)()
                _lib.check(self._lib.hvd_hasher_finish_autocrop(self._handle, hashes.ctypes.data, quality.ctypes.data, n,
                                                                C.byref(got), rect))
                self.rect = tuple(int(v) for v in rect)
            else:
                _lib.check(finish(self._handle, hashes.ctypes.data, quality.ctypes.data, n, C.byref(got)))
            assert got.value == n
            hashes, quality = hashes[:n], quality[:n]
            return hashes[quality >= QUALITY_TOLERANCE]
        finally:
            self.close()

    def finish(self) -> VpdqHash:
        """The video hash (vpdqpy.py:119); on a dihedral hasher its identity variant. Ends the hasher."""
        kept = self._drain()
        if kept is None:
            return VpdqHash(b"")
        return VpdqHash((kept if self._transforms is None else kept[:, 0]).tobytes())

    def finish_transformed(self) -> dict:
        """{transform name: VpdqHash} for the names given as ``transforms``, every variant over the same kept frames
        (what ``Vpdq.computeTransformedHashes`` returns). Ends the hasher."""
        if self._transforms is None:
            raise RuntimeError("finish_transformed() on a plain hasher: create it with transforms=")
        kept = self._drain()
        if kept is None:
            return {t: VpdqHash(b"") for t in self._transforms}
        return {t: VpdqHash(kept[:, TRANSFORMS.index(t)].tobytes()) for t in self._transforms}

    def close(self) -> None:
        if self._handle is not None:
            self._lib.hvd_hasher_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hash_frames(frames: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Batch entry point: uint8[n,h,w] (gray) or uint8[n,h,w,3] (rgb24) ->
    (hashes uint8[n,32], quality int32[n]). No quality filtering."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    lib = _lib.ensure()
    if frames.ndim == 3:
        fn = lib.hvd_pdq_hash_frames_gray_u8
    elif frames.ndim == 4 and frames.shape[3] == 3:
        fn = lib.hvd_pdq_hash_frames_rgb24_u8
    else:
        raise ValueError("frames must be uint8[n,h,w] or uint8[n,h,w,3]")
    n, h, w = frames.shape[:3]
    hashes = np.zeros((n, BYTES_PER_PDQ_HASH), dtype=np.uint8)
    quality = np.zeros(n, dtype=np.int32)
    _lib.check(fn(frames.ctypes.data, n, h, w, hashes.ctypes.data, quality.ctypes.data))
    return hashes, quality


# Content-rectangle PDQ (include/hvd_mi355x.h): bars are left out of the hash. The rule that tells bar from
# picture is one value, a RectRule, from the keywords of a call down to the native entry:
#   black      black bars (letterbox / pillarbox): a pixel is bright iff max(R, G, B) > black_level
#   color     bars that are not black: a pixel is content iff it differs from its video's bar colour by more than
#                          bar_level on some channel (include/hvd_mi355x.h: hvd_dev_bar_colors)
#   detail    bars that are smooth: a row is content iff it holds >= min_detail horizontal neighbour differences
#                          above detail_level, a column likewise with vertical ones (hvd_dev_content_rects_detail)
class _DetailRule:
    """What a RectRule of the detail kind holds in the colour's place."""

    def __repr__(self):
        return "DETAIL"


DETAIL = _DetailRule()


# A kind of rule: the keywords of its level and count with their defaults and ranges, the words of the level's range message
# (level_one_message: the level's type and range share one message, raised before the count is looked at), and its native
# entries -- hvd_pdq_hash_frames_<stem>_<format>, hvd_dev_content_rects<dev>, hvd_hasher_create_autocrop<dev>.
_RectKind = namedtuple("_RectKind", "level count level_default count_default level_range count_range why level_one_message stem dev")
_RECT_KINDS = {  # (the detail defaults are unverified on real video)
    "black": _RectKind("black_level", "min_bright", 16, 1, (0, 254), (1, 2**31 - 1),
                       "a pixel is bright iff max(R, G, B) > black_level", False, "autocrop", ""),
    "color": _RectKind("bar_level", "min_bright", 16, 1, (0, 254), (1, 2**31 - 1),
                       "a pixel is content iff it differs from the bar colour by more than bar_level on some channel", True,
                       "barcolor", "_color"),
    "detail": _RectKind("detail_level", "min_detail", 8, 8, (0, 254), (1, 2**31 - 1),
                        "two neighbours differ iff some channel differs by more than detail_level", False, "detail", "_detail"),
}
_KIND_KEYS = {"black": {"black_level", "min_bright"}, "color": {"bar_color", "bar_level"},
              "detail": {"detail", "detail_level", "min_detail"}}


class RectRule(NamedTuple):
    """The rule that finds a video's content rectangle: (level, count, colour). colour None is the black rule, DETAIL the
    detail rule, anything else ("auto", an int, a 3-tuple or an array [V, channels]) the bar colour of the colour rule.
    Equal to the plain 3-tuple of its fields."""
    level: int
    count: int
    colour: object = None

    @property
    def kind(self) -> str:
        """ "black", "color" or "detail": a key of the table of kinds."""
        if self.colour is None:
            return "black"
        return "detail" if self.colour is DETAIL else "color"

    def kwargs(self) -> dict:
        """The keywords of `hash_frames_autocrop` / `content_rects` that state this rule."""
        k = _RECT_KINDS[self.kind]
        stated = {k.level: self.level, k.count: self.count}
        if self.kind == "detail":
            stated["detail"] = True
        elif self.kind == "color":
            stated["bar_color"] = self.colour
        return stated


def rule_kwargs(rule) -> dict:
    """`RectRule.kwargs` of what `autocrop_rule` returned (not None), or of the plain tuple (level, count, colour)."""
    return RectRule(*rule).kwargs()


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _check_levels(kind: str, level, count) -> tuple[int, int]:
    """(level, count) of a rule of `kind` as ints, or the ValueError that names the keyword."""
    k = _RECT_KINDS[kind]
    lo, hi = k.level_range
    if k.level_one_message and (not _is_int(level) or not lo <= level <= hi):
        raise ValueError(f"{k.level} must be an integer in {lo}..{hi} ({k.why}), got {level!r}")
    for name, v in ((k.level, level), (k.count, count)):
        if not _is_int(v):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not lo <= level <= hi:
        raise ValueError(f"{k.level} must be in {lo}..{hi} ({k.why}), got {level}")
    if not k.count_range[0] <= count <= k.count_range[1]:
        raise ValueError(f"{k.count} must be >= {k.count_range[0]}, got {count}")
    return int(level), int(count)


_RULE_DEFAULTS = dict(black_level=16, min_bright=1, bar_color=None, bar_level=None, detail=False, detail_level=None,
                      min_detail=None)


def rect_rule(black_level=16, min_bright=1, bar_color=None, bar_level=None, detail=False, detail_level=None, min_detail=None,
              stated=None) -> RectRule:
    """The one parser of the rule's keywords, as `content_rects`, `hash_frames_autocrop` and
    `pipeline.hash_frames_autocrop_on_device` take them. bar_color not None is the colour rule with `bar_level` (default 16)
    and `min_bright`; detail=True the detail rule with `detail_level` (default 8, unverified) and `min_detail` (default 8,
    unverified); else the black rule with `black_level` and `min_bright`. A keyword of another rule beside the chosen one is a
    ValueError that names both. stated: the keywords the caller stated, in the order the messages name them (None: those
    that do not hold their default, in the order above; `autocrop_rule` passes the keys of its dict)."""
    kw = dict(black_level=black_level, min_bright=min_bright, bar_color=bar_color, bar_level=bar_level, detail=detail,
              detail_level=detail_level, min_detail=min_detail)
    if stated is None:
        stated = [name for name, v in kw.items() if v is not _RULE_DEFAULTS[name] and not (_is_int(v) and v == _RULE_DEFAULTS[name])]
    if detail is not True and detail is not False:
        raise ValueError(f"detail must be True or False, got {detail!r}")
    if detail:
        for name in stated:
            if name not in _KIND_KEYS["detail"]:
                raise ValueError(f"detail and {name} cannot be combined: the detail rule's parameters are detail_level and min_detail")
        k = _RECT_KINDS["detail"]
        return RectRule(*_check_levels("detail", k.level_default if detail_level is None else detail_level,
                                       k.count_default if min_detail is None else min_detail), DETAIL)
    for name, v in (("detail_level", detail_level), ("min_detail", min_detail)):
        if v is not None:
            raise ValueError(f"{name} needs detail=True (the detail rule, DESIGN 4.16)")
    if bar_color is None:
        if _KIND_KEYS["color"] & set(stated):
            raise ValueError("bar_level needs bar_color (the black rule's level is black_level)")
        return RectRule(*_check_levels("black", black_level, min_bright), None)
    if "black_level" in stated:
        raise ValueError("black_level and bar_color cannot be combined: the level of the bar-colour rule is bar_level")
    return RectRule(*_check_levels("color", _RECT_KINDS["color"].level_default if bar_level is None else bar_level, min_bright),
                    bar_color)


def autocrop_rule(autocrop) -> RectRule | None:
    """The `autocrop` argument of the video-level calls -> None when it is off (None / False), else its RectRule: `rect_rule`
    behind the check of the dict's shape. True is the black rule at its defaults (16, 1); a dict may hold ``black_level`` /
    ``min_bright`` (the black rule), ``bar_color`` ("auto", an int, a 3-tuple or an array [V, channels]) with ``bar_level``
    (default 16) / ``min_bright`` (the colour rule; ``black_level`` beside ``bar_color`` is a ValueError, and so is
    ``bar_level`` without it; the colour's shape is checked where the frames are known), or ``detail`` True with
    ``detail_level`` (default 8, unverified) / ``min_detail`` (default 8, unverified) (the detail rule; any key
    of the other rules beside it is a ValueError that names both, and so are ``detail_level`` / ``min_detail`` without
    ``detail``; ``"detail": False`` states the default). Argument errors are raised here, before any device work."""
    if autocrop is None or autocrop is False:
        return None
    if autocrop is True:
        autocrop = {}
    keys = set(autocrop) if isinstance(autocrop, dict) else None
    if keys is None or keys - set(_RULE_DEFAULTS):
        shape = "autocrop must be True / False or a dict with the keys black_level and min_bright"
        if keys is not None and keys & (_KIND_KEYS["color"] | _KIND_KEYS["detail"]):
            shape += ", or bar_color, bar_level and min_bright"
        if keys is not None and keys & _KIND_KEYS["detail"]:
            shape += ", or detail, detail_level and min_detail"
        raise ValueError(shape)
    return rect_rule(**autocrop, stated=sorted(keys))


def autocrop_params(autocrop) -> tuple[int, int] | None:
    """`autocrop_rule` for a call site that takes the black rule only: None when `autocrop` is off (None / False); else
    (black_level, min_bright) from True (the defaults 16, 1) or a dict with those two keys."""
    if isinstance(autocrop, dict) and set(autocrop) - _KIND_KEYS["black"]:
        raise ValueError("autocrop must be True / False or a dict with the keys black_level and min_bright")
    rule = autocrop_rule(autocrop)
    return None if rule is None else (rule.level, rule.count)


def _frames_args(frames, offsets):
    """frames as a contiguous uint8[n,h,w] / uint8[n,h,w,3] and the int64[V+1] CSR of its videos (None: one video)."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or not (frames.ndim == 3 or (frames.ndim == 4 and frames.shape[3] == 3)):
        raise ValueError("frames must be uint8[n,h,w] or uint8[n,h,w,3]")
    frames = np.ascontiguousarray(frames)
    n = frames.shape[0]
    if offsets is None:
        offsets = np.array([0, n], dtype=np.int64)
    else:
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or offsets[-1] != n or np.any(np.diff(offsets) < 0):
            raise ValueError(f"offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = {n}")
    return frames, offsets


def _pack_bar_color(bar_color, V: int, channels: int) -> np.ndarray | None:
    """None for "auto"; else int32[V] = c0 | c1 << 8 | c2 << 16 from an int (every channel), a sequence of `channels` ints (one
    colour for all videos) or an array [V, channels] (gray: also [V])."""
    if isinstance(bar_color, str):
        if bar_color != "auto":
            raise ValueError(f"bar_color must be 'auto', an int, a 3-tuple or an array [V, channels], got {bar_color!r}")
        return None
    c = np.asarray(bar_color)
    if c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"bar_color must hold integers in 0..255, got {bar_color!r}")
    if c.size and (c.min() < 0 or c.max() > 255):
        raise ValueError(f"bar_color must hold integers in 0..255, got {bar_color!r}")
    if c.ndim == 0:
        c = np.full((V, channels), int(c))
    elif c.shape == (channels,) and not (channels == 1 and V == 1):
        c = np.broadcast_to(c, (V, channels))
    elif channels == 1 and c.shape == (V,):
        c = c.reshape(V, 1)
    elif c.shape != (V, channels):
        raise ValueError(f"bar_color must be an int, {channels} ints or an array [V, channels] = [{V}, {channels}], got shape {c.shape}")
    c = c.astype(np.int32).reshape(V, channels)
    return np.ascontiguousarray(sum(c[:, k] << (8 * k) for k in range(channels)), dtype=np.int32).reshape(V)


def _unpack_bar_colors(packed: np.ndarray, channels: int) -> np.ndarray:
    return np.stack([(packed >> (8 * k)) & 0xFF for k in range(channels)], axis=1).astype(np.uint8)


def enqueue_rects(lib, rule: RectRule, packed, d_frames, n: int, h: int, w: int, channels: int, d_offsets, V: int, d_rects, temp,
                  run=lambda fn: fn()):
    """The rectangle step of `rule` on n frames that sit in HBM: its kind's hvd_dev_content_rects entry, enqueued on the
    library stream. d_frames, d_offsets, d_rects: device pointers. The colour kind takes the colours from `packed`
    (`_pack_bar_color`) or, where that is None ("auto"), finds them first (hvd_dev_bar_colors); d_rects None stops there
    (`bar_colors`). temp(DeviceBuffer) -> that buffer, which the caller frees once the work is done; run(fn): what the
    native calls run inside (a stage timer). -> the DeviceBuffer of the colours int32[V] (colour kind), else None."""
    entry = getattr(lib, "hvd_dev_content_rects" + _RECT_KINDS[rule.kind].dev)
    if rule.kind != "color":
        run(lambda: _lib.check(entry(d_frames, n, h, w, channels, d_offsets, V, rule.level, rule.count, d_rects)))
        return None
    d_col = temp(_lib.DeviceBuffer(4 * max(V, 1)) if packed is None else _lib.DeviceBuffer.from_array(packed))
    d_acc = None
    if packed is None:
        sb = C.c_size_t(0)
        _lib.check(lib.hvd_bar_colors_scratch_bytes(V, C.byref(sb)))
        d_acc = temp(_lib.DeviceBuffer(max(sb.value, 1)))

    def colour_rects():
        if d_acc is not None:
            _lib.check(lib.hvd_dev_bar_colors(d_frames, n, h, w, channels, d_offsets, V, rule.level, d_acc.ptr, d_col.ptr))
        if d_rects is not None:
            _lib.check(entry(d_frames, n, h, w, channels, d_offsets, V, d_col.ptr, rule.level, rule.count, d_rects))

    run(colour_rects)
    return d_col


def _rects_of_host_frames(rule: RectRule, packed, frames, offsets, want_rects: bool):
    """`enqueue_rects` on host frames, uploaded for the call. -> rects int32[V,4] (want_rects), or the colours int32[V]."""
    lib = _lib.ensure()
    n, h, w = frames.shape[:3]
    V = len(offsets) - 1
    bufs = []

    def temp(buf):
        bufs.append(buf)
        return buf

    try:
        d_fr = temp(_lib.DeviceBuffer.from_array(frames)) if n else None
        d_off = temp(_lib.DeviceBuffer.from_array(offsets))
        d_rc = temp(_lib.DeviceBuffer(16 * V)) if want_rects else None
        d_col = enqueue_rects(lib, rule, packed, d_fr.ptr if n else None, n, h, w, 1 if frames.ndim == 3 else 3, d_off.ptr, V,
                              d_rc.ptr if want_rects else None, temp)
        return d_rc.to_array(np.int32, V * 4).reshape(V, 4) if want_rects else d_col.to_array(np.int32, V)
    finally:
        for b in bufs:
            b.free()


def bar_colors(frames: np.ndarray, offsets=None, bar_level: int = 16) -> np.ndarray:
    """The automatic bar colour of every video, found on the device from the four corner pixels of all its frames:
    uint8[V, channels] in the byte order of the pixel; (0, ...) where the corners differ by more than bar_level (no uniform
    bars: the black rule) and for a video without frames. The rule is in include/hvd_mi355x.h (hvd_dev_bar_colors)."""
    level, _ = _check_levels("color", _RECT_KINDS["color"].level_default if bar_level is None else bar_level, 1)
    frames, offsets = _frames_args(frames, offsets)
    channels = 1 if frames.ndim == 3 else 3
    if len(offsets) == 1:
        return np.zeros((0, channels), dtype=np.uint8)
    return _unpack_bar_colors(_rects_of_host_frames(RectRule(level, 1, "auto"), None, frames, offsets, False), channels)


def content_rects(frames: np.ndarray, offsets=None, black_level: int = 16, min_bright: int = 1, bar_color=None,
                  bar_level=None, detail=False, detail_level=None, min_detail=None) -> np.ndarray:
    """The content rectangle of every video, found on the device: int32[V,4] = (top, left, height, width). frames:
    uint8[n,h,w] or uint8[n,h,w,3]; offsets: int64[V+1] CSR of the videos (None: one video). The rule is in
    include/hvd_mi355x.h (hvd_dev_content_rects).
    bar_color: None is that rule (black bars). "auto", an int, a 3-tuple or an array [V, channels] is the bar-colour rule
    (hvd_dev_bar_colors) with the level `bar_level` (default 16): bars of the video's colour are left out.
    detail=True is the detail rule (hvd_dev_content_rects_detail) with `detail_level` (default 8, unverified)
    and `min_detail` (default 8, unverified): smooth bars of any colour are left out; none of the other rules' keywords
    goes with it."""
    rule = rect_rule(black_level, min_bright, bar_color, bar_level, detail, detail_level, min_detail)
    frames, offsets = _frames_args(frames, offsets)
    V = len(offsets) - 1
    packed = _pack_bar_color(rule.colour, V, 1 if frames.ndim == 3 else 3) if rule.kind == "color" else None
    if V == 0:
        return np.zeros((0, 4), dtype=np.int32)
    return _rects_of_host_frames(rule, packed, frames, offsets, True)


def hash_frames_autocrop(frames: np.ndarray, offsets=None, black_level: int = 16, min_bright: int = 1, bar_color=None,
                         bar_level=None, detail=False, detail_level=None,
                         min_detail=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`hash_frames` inside every video's content rectangle: (hashes uint8[n,32], quality int32[n], rects int32[V,4]).
    A frame's hash and quality are the plain PDQ hash and quality of frames[f, top:top+height, left:left+width] under its
    video's rectangle. offsets: int64[V+1] CSR of the videos (None: one video). No quality filtering.
    bar_color / bar_level: as `content_rects` -- the rectangle then leaves out bars of the video's colour (`bar_colors`
    returns what "auto" finds).
    detail / detail_level / min_detail: as `content_rects` -- the rectangle then leaves out smooth bars of any colour."""
    rule = rect_rule(black_level, min_bright, bar_color, bar_level, detail, detail_level, min_detail)
    frames, offsets = _frames_args(frames, offsets)
    n, h, w = frames.shape[:3]
    V = len(offsets) - 1
    colours_in = colours_out = ()  # the colour kind's entries take the caller's colours and return the ones used
    if rule.kind == "color":
        packed = _pack_bar_color(rule.colour, V, 1 if frames.ndim == 3 else 3)
        used = np.zeros(V, dtype=np.int32)
        colours_in, colours_out = (None if packed is None else packed.ctypes.data,), (used.ctypes.data,)
    lib = _lib.ensure()
    hashes = np.zeros((n, BYTES_PER_PDQ_HASH), dtype=np.uint8)
    quality = np.zeros(n, dtype=np.int32)
    rects = np.zeros((V, 4), dtype=np.int32)
    fn = getattr(lib, f"hvd_pdq_hash_frames_{_RECT_KINDS[rule.kind].stem}_{'gray_u8' if frames.ndim == 3 else 'rgb24_u8'}")
    _lib.check(fn(frames.ctypes.data, n, h, w, offsets.ctypes.data, V, *colours_in, rule.level, rule.count, hashes.ctypes.data,
                  quality.ctypes.data, rects.ctypes.data, *colours_out))
    return hashes, quality, rects


# Dihedral PDQ (include/hvd_mi355x.h): the hashes of the frame's mirror images and rotations, in the
# kernel's output order -- TRANSFORMS[k] is what hash_frames_dihedral(frames)[0][:, k] hashes. Names of the physical
# transform of the 64x64 luma A (rows top to bottom; rotations as numpy's rot90): A, A[:, ::-1], A[::-1, :],
# A[::-1, ::-1], A.T, A[::-1, ::-1].T, rot90(A, 1), rot90(A, -1).
TRANSFORMS = ("identity", "flip_h", "flip_v", "rot180", "transpose", "antitranspose", "rot90_ccw", "rot90_cw")


def hash_frames_dihedral(frames: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Dihedral counterpart of `hash_frames`: uint8[n,h,w] (gray) or uint8[n,h,w,3] (rgb24) ->
    (hashes uint8[n,8,32] in TRANSFORMS order, quality int32[n]). hashes[:, 0] equals hash_frames(frames)[0]; one
    quality per frame serves all 8. No quality filtering. Strict DCT mode only (the "fma" mode raises HvdError)."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    lib = _lib.ensure()
    if frames.ndim == 3:
        fn = lib.hvd_pdq_hash_frames_dihedral_gray_u8
    elif frames.ndim == 4 and frames.shape[3] == 3:
        fn = lib.hvd_pdq_hash_frames_dihedral_rgb24_u8
    else:
        raise ValueError("frames must be uint8[n,h,w] or uint8[n,h,w,3]")
    n, h, w = frames.shape[:3]
    hashes = np.zeros((n, len(TRANSFORMS), BYTES_PER_PDQ_HASH), dtype=np.uint8)
    quality = np.zeros(n, dtype=np.int32)
    _lib.check(fn(frames.ctypes.data, n, h, w, hashes.ctypes.data, quality.ctypes.data))
    return hashes, quality


# Crop-ladder PDQ (include/hvd_mi355x.h): every frame hashed under the full frame and under a short list of
# rectangles, so that an aspect-ratio re-crop ("crop to fill") matches its source under the rectangle it kept. A rung
# (axis, num, den) keeps the centre (side * num) // den pixels of that axis and all of the other one; CROP_NAMES names the
# listed rungs the way TRANSFORMS names the dihedral variants: 16:9 -> 4:3, 1:1, 9:16 on the width, the same on the height.
CROP_RUNGS = {"w3/4": ("w", 3, 4), "w9/16": ("w", 9, 16), "w81/256": ("w", 81, 256),
              "h3/4": ("h", 3, 4), "h9/16": ("h", 9, 16), "h81/256": ("h", 81, 256)}
CROP_NAMES = tuple(CROP_RUNGS)
CROP_SETS = {"landscape": CROP_NAMES[:3], "portrait": CROP_NAMES[3:], "aspect": CROP_NAMES}
MAX_CROPS = 7  # HVD_MAX_CROPS


def _crop_items(crops) -> list:
    """`crops` as crop_ladder takes it -> [(name, rung or pixel rectangle)], in list order."""
    if isinstance(crops, str):
        if crops not in CROP_SETS:
            raise ValueError(f"unknown crop set {crops!r}; expected one of {sorted(CROP_SETS)}, or a tuple of rungs "
                             f"(names from {CROP_NAMES}, (axis, num, den)) or pixel rectangles (top, left, height, width)")
        crops = CROP_SETS[crops]
    items = []
    for c in crops:
        if isinstance(c, str):
            if c not in CROP_RUNGS:
                raise ValueError(f"unknown crop rung {c!r}; expected names from {CROP_NAMES}")
            items.append((c, CROP_RUNGS[c]))
            continue
        c = tuple(c)
        if len(c) == 3 and c[0] in ("w", "h"):
            axis, num, den = c[0], int(c[1]), int(c[2])
            if not 1 <= num <= den:
                raise ValueError(f"crop rung {c!r}: need 1 <= num <= den")
            items.append((f"{axis}{num}/{den}", (axis, num, den)))
        elif len(c) == 4 and not isinstance(c[0], str):
            rect = tuple(int(x) for x in c)
            items.append(("r{},{},{},{}".format(*rect), rect))
        else:
            raise ValueError(f"crop {c!r} is neither a rung (axis, num, den) nor a rectangle (top, left, height, width)")
    if not 1 <= len(items) <= MAX_CROPS:
        raise ValueError(f"a crop list holds 1..{MAX_CROPS} crops, got {len(items)}")
    return items


def crop_names(crops="aspect", unique: bool = False) -> tuple:
    """The names of a crop list, in list order (what crop_ladder(h, w, crops)[0] is at any geometry). unique=True: ValueError
    if a crop is listed twice -- legal for the hashing entries, but a result keyed by name would hold one of the two."""
    names = tuple(name for name, _ in _crop_items(crops))
    if unique and len(set(names)) != len(names):
        raise ValueError(f"a crop is listed twice in {names}: variants are keyed by name")
    return names


def crop_ladder(h: int, w: int, crops="aspect") -> tuple[tuple, np.ndarray]:
    """(names, int32[K,4] = (top, left, height, width)) of a crop list in an h x w frame. crops: "landscape" (w3/4, w9/16,
    w81/256: a 16:9 frame cut to 4:3, 1:1, 9:16), "portrait" (the same on the height), "aspect" (all six), or a tuple of
    rung names, rungs (axis, num, den) and explicit pixel rectangles, taken as given (1..7 of them). A rung ("w", num, den)
    keeps ww = (w * num) // den columns at left = (w - ww) // 2 and all rows; ("h", num, den) the same on the other axis.
    ValueError for a rung whose kept side would be below 64 and for a rectangle that is not inside the frame with both
    sides >= 64. Only these centre crops are found; an off-centre crop needs its explicit rectangle."""
    h, w = int(h), int(w)
    rects = []
    for name, c in _crop_items(crops):
        if len(c) == 3:
            axis, num, den = c
            if axis == "w":
                ww = (w * num) // den
                rect = (0, (w - ww) // 2, h, ww)
            else:
                hh = (h * num) // den
                rect = ((h - hh) // 2, 0, hh, w)
            if min(rect[2], rect[3]) < 64:
                raise ValueError(f"crop rung {name} keeps {rect[2]} x {rect[3]} of a {h} x {w} frame: both sides must be >= 64")
        else:
            rect = c
            top, left, hh, ww = rect
            if top < 0 or left < 0 or hh < 64 or ww < 64 or top + hh > h or left + ww > w:
                raise ValueError(f"crop rectangle {rect} must lie inside the {h} x {w} frame with both sides >= 64")
        rects.append(rect)
    return tuple(n for n, _ in _crop_items(crops)), np.array(rects, dtype=np.int32).reshape(-1, 4)


def hash_frames_crops(frames: np.ndarray, crops="aspect") -> tuple[np.ndarray, np.ndarray, np.ndarray, tuple]:
    """Crop-ladder counterpart of `hash_frames`: uint8[n,h,w] (gray) or uint8[n,h,w,3] (rgb24) -> (hashes uint8[n,K+1,32],
    quality int32[n], crop_quality int32[n,K+1], names). Slot 0 is the full frame (hashes[:, 0] and quality equal
    hash_frames(frames)), slot k + 1 the plain PDQ hash and quality of frames[f, top:top+height, left:left+width] under
    crop k of `crop_ladder(h, w, crops)`; names[k] names it. No quality filtering. Both DCT modes."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or not (frames.ndim == 3 or (frames.ndim == 4 and frames.shape[3] == 3)):
        raise ValueError("frames must be uint8[n,h,w] or uint8[n,h,w,3]")
    frames = np.ascontiguousarray(frames)
    n, h, w = frames.shape[:3]
    names, rects = crop_ladder(h, w, crops)
    K = len(names)
    lib = _lib.ensure()
    fn = lib.hvd_pdq_hash_frames_crops_gray_u8 if frames.ndim == 3 else lib.hvd_pdq_hash_frames_crops_rgb24_u8
    hashes = np.zeros((n, 8, BYTES_PER_PDQ_HASH), dtype=np.uint8)
    quality = np.zeros(n, dtype=np.int32)
    crop_quality = np.zeros((n, 8), dtype=np.int32)
    _lib.check(fn(frames.ctypes.data, n, h, w, rects.ctypes.data, K, hashes.ctypes.data, quality.ctypes.data,
                  crop_quality.ctypes.data))
    return np.ascontiguousarray(hashes[:, :K + 1]), quality, np.ascontiguousarray(crop_quality[:, :K + 1]), names


def match_counts(a: bytes, b: bytes, distance_tolerance: int = 31) -> tuple[int, int]:
    """(q_hits, t_hits) for query a / target b, both concatenated 32-byte frame hashes."""
    a = bytes(a)
    b = bytes(b)
    if len(a) % BYTES_PER_PDQ_HASH or len(b) % BYTES_PER_PDQ_HASH:
        raise ValueError("hash byte strings must be multiples of 32 bytes")
    na, nb = len(a) // BYTES_PER_PDQ_HASH, len(b) // BYTES_PER_PDQ_HASH
    lib = _lib.ensure()
    q, t = C.c_int32(0), C.c_int32(0)
    _lib.check(lib.hvd_match_two(a if na else None, na, b if nb else None, nb, int(distance_tolerance),
                                 C.byref(q), C.byref(t)))
    return q.value, t.value


def matchHashBytes(a: bytes, b: bytes, distance_tolerance: int) -> float:
    """db/vptree.py:31 call shape: similarity in [0,100] from two raw BLOBs."""
    if not _warned_unverified:
        warn_unverified_policies()
    max_dist = frame_max_dist(distance_tolerance)
    if max_dist < 0:
        if len(a) % BYTES_PER_PDQ_HASH or len(b) % BYTES_PER_PDQ_HASH:
            raise ValueError("hash byte strings must be multiples of 32 bytes")
        return 0.0
    q, t = match_counts(a, b, max_dist)
    return percent_from_hits(q, t, len(a) // BYTES_PER_PDQ_HASH, len(b) // BYTES_PER_PDQ_HASH)


def matchHash(query: VpdqHash, target: VpdqHash, distance_tolerance: int) -> float:
    """vpdqpy/vpdqpy.py:56 call shape."""
    return matchHashBytes(query.bytes, target.bytes, distance_tolerance)
