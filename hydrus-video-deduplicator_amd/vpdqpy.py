"""Host-side mirror of the reference facade ``vpdqpy/vpdqpy.py`` (class Vpdq), bound to the
MI355X kernels instead of ``hvdaccelerators``. Same names, argument meaning and error
behaviour; video *decoding* (PyAV/FFmpeg, vpdqpy.py:58-101) is out of scope, so
``computeHash`` takes pre-decoded frames (or an iterable of frame byte strings) in the
format ``frame_extract_pyav`` yields: 512x512 packed rgb24 (vpdqpy.py:90-95)."""

from __future__ import annotations

import os
from collections.abc import Iterable

import numpy as np

from . import vpdq

# The dimensions of the image after downscaling for pdq (vpdqpy.py:23)
DOWNSCALE_DIMENSIONS = 512

VpdqHash = vpdq.VpdqHash


def hashed_frame_stride(average_rate) -> int:
    """Every how-many-th decoded frame the reference hashes (vpdqpy.py:72-77): ``round(average_rate)`` of the
    stream's average frame rate -- Python's round, so a Fraction of exactly k + 1/2 goes to the even neighbour,
    as it does there -- and 1 (every frame) when the rate is None or below 1 (small GIFs)."""
    if average_rate is None or average_rate < 1:
        return 1
    return round(average_rate)


def select_frames(frames, average_rate, bad_frame_errors: tuple = ()):
    """The frame-selection rule of ``frame_extract_pyav`` (vpdqpy.py:72-77,85-101) for a decoder-side caller:
    yield the frames whose DECODE index is a multiple of ``hashed_frame_stride(average_rate)``.

    `frames` is any iterable of decoded frames in decode order. An exception of a type listed in
    `bad_frame_errors` (the reference: ``av.error.InvalidDataError``) raised while fetching a frame skips that
    frame but still advances the index (vpdqpy.py:99-101), so the frames after it keep their phase. Which frames
    are hashed is part of the video hash: feed ``Vpdq.computeHash`` / ``VideoHasher.hash_frame`` from this."""
    stride = hashed_frame_stride(average_rate)
    it = iter(frames)
    frame_index = 0
    while True:
        try:
            frame = next(it)
            if frame_index % stride == 0:
                yield frame
            frame_index += 1
        except StopIteration:
            break
        except bad_frame_errors:
            frame_index += 1


def selected_frame_indices(n_decoded: int, average_rate) -> np.ndarray:
    """Decode indices `select_frames` keeps out of n_decoded good frames (array form: ``frames[idx]``)."""
    return np.arange(0, max(0, int(n_decoded)), hashed_frame_stride(average_rate), dtype=np.int64)


class Vpdq:
    @staticmethod
    def match_hash(query_features: VpdqHash, target_features: VpdqHash, distance_tolerance: float = 31.0):
        """Get the similarity of two videos by comparing their list of features (vpdqpy.py:49-56)."""
        return vpdq.matchHash(query_features, target_features, int(distance_tolerance))

    @staticmethod
    def align(phash_a, phash_b, slack: int = 1):
        """Where two video hashes line up in time: the one ``search.align_videos`` record of the pair (a = 0, b = 1; best
        offset p_b = p_a + offset, aligned frames per side and their first / last index). VpdqHash or bytes."""
        from . import search

        frames, offsets, _ = search.pack_hashes((phash_a, phash_b))
        return search.align_videos(frames, offsets, [(0, 1)], slack=slack)[0]

    @staticmethod
    def align_segments(phash_a, phash_b, slack: int = 1, max_segments: int = 8, min_band_votes: int = 1):
        """Where the pieces of two video hashes line up in time -- a reel or re-cut against its source: the one
        ``search.align_segments`` record of the pair (a = 0, b = 1; up to max_segments offsets, seg[0] is ``align``'s).
        VpdqHash or bytes."""
        from . import search

        frames, offsets, _ = search.pack_hashes((phash_a, phash_b))
        return search.align_segments(frames, offsets, [(0, 1)], slack=slack, max_segments=max_segments,
                                     min_band_votes=min_band_votes)[0]

    @staticmethod
    def align_rates(phash_a, phash_b, rates=None, slack: int = 1):
        """Where two video hashes line up in time when one of them was sped up or slowed down: the one
        ``search.align_rates`` record of the pair (a = 0, b = 1; the best-fitting rate of `rates`, default
        ``search.DEFAULT_RATES``, p_b = (rate_num / rate_den) p_a + offset / rate_den). VpdqHash or bytes."""
        from . import search

        frames, offsets, _ = search.pack_hashes((phash_a, phash_b))
        return search.align_rates(frames, offsets, [(0, 1)], rates=search.DEFAULT_RATES if rates is None else rates,
                                  slack=slack)[0]

    @staticmethod
    def align_rate_segments(phash_a, phash_b, rates=None, slack: int = 1, max_segments: int = 8):
        """Where the pieces of two video hashes line up in time when the pieces were also sped up or slowed down -- a sped-up
        reel against its source: the one ``search.align_rate_segments`` record of the pair (a = 0, b = 1; up to max_segments
        lines, each at the best-fitting rate of `rates`, default ``search.DEFAULT_RATES``). VpdqHash or bytes."""
        from . import search

        frames, offsets, _ = search.pack_hashes((phash_a, phash_b))
        return search.align_rate_segments(frames, offsets, [(0, 1)], rates=search.DEFAULT_RATES if rates is None else rates,
                                          slack=slack, max_segments=max_segments)[0]

    @staticmethod
    def align_signed(phash_a, phash_b, rates=None, slack: int = 1, max_segments: int = 8):
        """Where the pieces of two video hashes line up in time when a piece may run BACKWARDS -- a reversed clip or a
        "rewind" piece of a reel against its source: the one ``search.align_signed`` record of the pair (a = 0, b = 1; up to
        max_segments lines, each at the best-fitting rate of `rates`, default ``search.REVERSED_RATES``; rate_num < 0: b runs
        backwards against a). VpdqHash or bytes."""
        from . import search

        frames, offsets, _ = search.pack_hashes((phash_a, phash_b))
        return search.align_signed(frames, offsets, [(0, 1)], rates=search.REVERSED_RATES if rates is None else rates,
                                   slack=slack, max_segments=max_segments)[0]

    @staticmethod
    def align_loops(phash_a, phash_b, rates=None, slack: int = 1, max_rounds: int = 64, min_band_votes: int = 1):
        """Where a LOOPED clip a -- a moment repeated, a ping-pong / boomerang loop -- lines up with its source b: the one
        ``search.align_loops`` record of the pair (a = 0, b = 1; up to max_rounds lines, each at the best-fitting rate of
        `rates`, default ``search.REVERSED_RATES``; a frame of b may serve any number of lines, a frame of a serves one; the
        first eight lines are stored as segments). VpdqHash or bytes."""
        from . import search

        frames, offsets, _ = search.pack_hashes((phash_a, phash_b))
        return search.align_loops(frames, offsets, [(0, 1)], rates=search.REVERSED_RATES if rates is None else rates,
                                  max_rounds=max_rounds, min_band_votes=min_band_votes, slack=slack)[0]

    select_frames = staticmethod(select_frames)

    @staticmethod
    def computeHash(frames, num_threads: int = 0, width: int | None = None, height: int | None = None,
                    average_rate=None, all_decoded_frames: bool = False, autocrop=False) -> VpdqHash:
        """Perceptually hash a video given its decoded frames (vpdqpy.py:103-119 minus decode).

        frames: uint8[n,h,w,3] / uint8[n,h,w] array, or an iterable of per-frame byte strings
        (then width/height default to DOWNSCALE_DIMENSIONS, as the reference passes). By default `frames` are
        the frames to hash (what ``frame_extract_pyav`` yields); with ``all_decoded_frames=True`` they are EVERY
        decoded frame and the reference's selection rule is applied first (``select_frames(frames, average_rate)``).

        autocrop: True, or a dict with ``black_level`` / ``min_bright``, hashes an array of frames inside the video's content
        rectangle (``vpdq.hash_frames_autocrop``: black bars are left out) and applies the usual quality filter. A dict with
        ``bar_color`` ("auto", an int, a 3-tuple) / ``bar_level`` / ``min_bright`` leaves out bars of that colour instead
        (``vpdq.autocrop_rule``); ``{"detail": True}`` with optional ``detail_level`` / ``min_detail`` leaves out
        smooth bars of any colour -- blurred, gradient -- (DESIGN 4.16). The rectangle
        is known only after the last frame, so an iterable of frames cannot be hashed this way: pass the array form."""
        if frames is None:
            raise ValueError
        crop = vpdq.autocrop_rule(autocrop)
        if crop is not None and not isinstance(frames, np.ndarray):
            raise ValueError("autocrop needs the array form of the frames (uint8[n,h,w] or uint8[n,h,w,3]): the content "
                             "rectangle is known only after the last frame, so an iterable cannot be streamed")
        if all_decoded_frames and not isinstance(frames, (bytes, bytearray, memoryview, str, os.PathLike)):
            frames = (frames[selected_frame_indices(frames.shape[0], average_rate)] if isinstance(frames, np.ndarray)
                      else select_frames(frames, average_rate))
        if isinstance(frames, (bytes, bytearray, memoryview, str, os.PathLike)):
            # the reference's caller passes the ENCODED video (dedup.py:76) and decodes it with PyAV; decoding is
            # out of scope here, and iterating a bytes object would silently hash garbage
            raise ValueError("encoded video input (bytes / path) is not supported: decode first and pass the frames "
                             "(uint8[n,h,w,3] array or an iterable of per-frame byte strings)")
        average_fps = 1  # timestamps are discarded (vpdqpy.py:110-112)
        if isinstance(frames, np.ndarray):
            if frames.ndim not in (3, 4):
                raise ValueError("frames must be uint8[n,h,w] or uint8[n,h,w,3]")
            h, w = frames.shape[1], frames.shape[2]
            if crop is not None:
                hashes, quality, _ = vpdq.hash_frames_autocrop(frames, None, **crop.kwargs())
                return VpdqHash(hashes[quality >= vpdq.QUALITY_TOLERANCE].tobytes())
            hasher = vpdq.VideoHasher(average_fps, w, h, num_threads)
            flat = np.ascontiguousarray(frames, dtype=np.uint8).reshape(frames.shape[0], -1)
            for f in flat:
                hasher.hash_frame(f.data)
            return hasher.finish()
        if isinstance(frames, Iterable):
            w = DOWNSCALE_DIMENSIONS if width is None else width
            h = DOWNSCALE_DIMENSIONS if height is None else height
            hasher = vpdq.VideoHasher(average_fps, w, h, num_threads)
            for frame in frames:
                hasher.hash_frame(frame)
            return hasher.finish()
        raise ValueError("Failed to hash: invalid frames object type.")

    @staticmethod
    def computeTransformedHashes(frames, transforms="dihedral", width: int | None = None, height: int | None = None,
                                 average_rate=None, all_decoded_frames: bool = False) -> dict:
        """The video hashes of the video's mirror images / rotations: {transform name: VpdqHash}, for the names of
        `transforms` (a set name of ``search.transform_set`` -- "mirror", "flips", "dihedral" -- or a sequence of
        ``vpdq.TRANSFORMS`` names). Takes what ``computeHash`` takes; all variants come from one dihedral hashing pass
        and keep the SAME frames: the quality filter (>= QUALITY_TOLERANCE) is applied once, per frame.
        ``["identity"]`` equals ``computeHash(frames)``. An array goes through the batch entry
        (vpdq.hash_frames_dihedral); an iterable is streamed through a dihedral ``vpdq.VideoHasher``, so host memory
        stays bounded by its ring whatever the length of the video."""
        from .search import transform_set

        names = transform_set(transforms, require_identity=False)
        if frames is None:
            raise ValueError
        if isinstance(frames, (bytes, bytearray, memoryview, str, os.PathLike)):
            raise ValueError("encoded video input (bytes / path) is not supported: decode first and pass the frames "
                             "(uint8[n,h,w,3] array or an iterable of per-frame byte strings)")
        if all_decoded_frames:
            frames = (frames[selected_frame_indices(frames.shape[0], average_rate)] if isinstance(frames, np.ndarray)
                      else select_frames(frames, average_rate))
        if isinstance(frames, np.ndarray):
            if frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] != 3):
                raise ValueError("frames must be uint8[n,h,w] or uint8[n,h,w,3]")
            arr = frames
        elif isinstance(frames, Iterable):
            w = DOWNSCALE_DIMENSIONS if width is None else int(width)
            h = DOWNSCALE_DIMENSIONS if height is None else int(height)
            hasher = vpdq.VideoHasher(1, w, h, transforms=names)
            try:
                for frame in frames:
                    hasher.hash_frame(frame)
                return hasher.finish_transformed()
            finally:
                hasher.close()
        else:
            raise ValueError("Failed to hash: invalid frames object type.")
        if arr.shape[1] < 64 or arr.shape[2] < 64:
            raise ValueError("frames must be at least 64x64")
        hashes, quality = vpdq.hash_frames_dihedral(arr)
        kept = hashes[quality >= vpdq.QUALITY_TOLERANCE]
        return {t: VpdqHash(kept[:, vpdq.TRANSFORMS.index(t)].tobytes()) for t in names}

    @staticmethod
    def computeCroppedHashes(frames, crops="aspect") -> dict:
        """The video hashes of the video under the full frame and under every crop of `crops` (what ``vpdq.crop_ladder``
        takes): {"identity": VpdqHash, "w3/4": VpdqHash, ...}, from one crop-ladder hashing call
        (``vpdq.hash_frames_crops``). All variants keep the SAME frames: the quality filter (>= QUALITY_TOLERANCE) is
        applied once, on the full frame's quality, as ``computeTransformedHashes`` does. ``["identity"]`` equals
        ``computeHash(frames)``. frames: uint8[n,h,w] / uint8[n,h,w,3] array (the streaming form is not offered). The result
        is keyed by name, so a crop listed twice is a ValueError here (``vpdq.hash_frames_crops`` takes it)."""
        vpdq.crop_names(crops, unique=True)
        if not isinstance(frames, np.ndarray):
            raise ValueError("computeCroppedHashes needs the array form of the frames (uint8[n,h,w] or uint8[n,h,w,3])")
        hashes, quality, _, names = vpdq.hash_frames_crops(frames, crops)
        kept = hashes[quality >= vpdq.QUALITY_TOLERANCE]
        return {name: VpdqHash(kept[:, k].tobytes()) for k, name in enumerate(("identity",) + tuple(names))}

    @staticmethod
    def is_similar(vpdq_features1: VpdqHash, vpdq_features2: VpdqHash, threshold: float = 75.0) -> tuple[bool, float]:
        """Threshold is minimum similarity to be considered similar (vpdqpy.py:121-131)."""
        similarity = Vpdq.match_hash(query_features=vpdq_features1, target_features=vpdq_features2)
        return similarity >= threshold, similarity
