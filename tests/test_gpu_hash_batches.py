"""The batch loops of the host-buffer hashing entries (csrc/hvd_search.cpp: hash_in_batches, the autocrop entry's walk over
whole videos) with more than one batch. A batch stages at most 1 GiB of frames, so until hvd_debug_set("hash_staging_bytes")
no test could reach the second one. Every case hashes the same frames twice, under the default limit (one batch) and under a
small one, and the two results must be equal bit for bit; the one-batch result is the oracle's."""
import contextlib

import numpy as np
import pytest

import autocrop_helpers as A
import crops_helpers as H
from test_gpu_autocrop import join, paint
from test_gpu_dihedral import reference as dihedral_reference

pytestmark = pytest.mark.gpu

FILL = 0xA5


@contextlib.contextmanager
def staging_limit(gpu, nbytes):
    lib = gpu.ensure()
    gpu.check(lib.hvd_debug_set(b"hash_staging_bytes", nbytes))
    try:
        yield
    finally:
        gpu.check(lib.hvd_debug_set(b"hash_staging_bytes", 0))


def noise(seed, n, h, w, ch):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if ch == 1 else (n, h, w, 3), dtype=np.uint8)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- plain and dihedral ----

# 64x64 gray (no scratch), 16 frames a batch: 40 = 16 + 16 + a tail of 8, 33: a tail of 1, 32: no tail; 96x128 rgb (the
# down-sampler and its scratch), 4 frames a batch: 4 + 4 + 2
PLAIN = [(40, 64, 64, 1, 16), (33, 64, 64, 1, 16), (32, 64, 64, 1, 16), (10, 96, 128, 3, 4)]


@pytest.mark.parametrize("n,h,w,ch,per_batch", PLAIN, ids=[f"{n}x{h}x{w}x{ch}" for n, h, w, ch, _ in PLAIN])
def test_plain_and_dihedral_in_batches(gpu, hvd, oracle, n, h, w, ch, per_batch):
    fr = noise(n, n, h, w, ch)
    one = hvd.vpdq.hash_frames(fr)
    one8 = hvd.vpdq.hash_frames_dihedral(fr)
    with staging_limit(gpu, per_batch * h * w * ch):
        many = hvd.vpdq.hash_frames(fr)
        many8 = hvd.vpdq.hash_frames_dihedral(fr)
    assert same(many, one), np.flatnonzero((many[0] != one[0]).any(1))[:8]
    assert same(many8, one8), np.flatnonzero((many8[0] != one8[0]).any(axis=(1, 2)))[:8]
    assert same(one, oracle.hash_frames(fr, num_threads=4))
    assert same(one8, dihedral_reference(oracle, fr, num_threads=4))


# ---- crop ladder ----

def host_crops(gpu, frames, rects, with_crop_quality):
    """The host-buffer entry on output buffers pre-filled with FILL -> (uint8[n,8,32], int32[n], int32[n,8])."""
    lib = gpu.ensure()
    n, h, w = frames.shape[:3]
    h8, q, cq = np.full((n, 8, 32), FILL, np.uint8), np.full(n, FILL, np.int32), np.full((n, 8), FILL, np.int32)
    gpu.check(lib.hvd_pdq_hash_frames_crops_gray_u8(frames.ctypes.data, n, h, w, rects.ctypes.data, rects.shape[0], h8.ctypes.data,
                                                    q.ctypes.data, cq.ctypes.data if with_crop_quality else None))
    return h8, q, cq


# "aspect" keeps 81/256 of a side, which must stay >= 64: it exists from 203 pixels a side on. 96x128 takes the rungs of it
# that fit there; 208x224 the whole set.
CROPS = [(96, 128, ("w3/4", "w9/16", "h3/4")), (208, 224, "aspect")]


@pytest.mark.parametrize("with_crop_quality", [True, False], ids=["crop_quality", "no_crop_quality"])
@pytest.mark.parametrize("h,w,crops", CROPS, ids=["96x128", "208x224-aspect"])
def test_crop_ladder_in_batches(gpu, hvd, oracle, h, w, crops, with_crop_quality):
    fr = noise(7, 10, h, w, 1)
    names, rects = hvd.vpdq.crop_ladder(h, w, crops)
    K = len(names)
    one = host_crops(gpu, fr, rects, with_crop_quality)
    with staging_limit(gpu, 4 * h * w):
        many = host_crops(gpu, fr, rects, with_crop_quality)
    assert same(many, one)
    want_h, want_q = H.oracle_crops(oracle, fr, rects)
    assert np.array_equal(one[0][:, :K + 1], want_h) and np.array_equal(one[1], want_q[:, 0])
    if with_crop_quality:
        assert np.array_equal(one[2][:, :K + 1], want_q)
    else:
        assert (one[2] == FILL).all(), "no crop qualities were asked for"


# ---- autocrop ----

H96, W128 = 96, 128
BOXES = [(8, 0, 80, 128), (0, 16, 96, 96), (0, 0, H96, W128), (5, 9, 70, 101), (12, 20, 64, 64), (3, 0, 90, 128), None]


def barred_videos(lengths, seed, boxes=BOXES):
    """Gray 96x128 videos of these lengths, video v with bars around boxes[v] (None: all dark; the frame: no bars)."""
    return join([paint(n, H96, W128, 1, boxes[v % len(boxes)], seed + v) for v, n in enumerate(lengths)])


def raw_autocrop(gpu, frames, off):
    """(rc, hashes, quality, rects) of the host-buffer entry on output buffers pre-filled with FILL."""
    lib = gpu.ensure()
    n, V = len(frames), len(off) - 1
    hs, q, rc = np.full((n, 32), FILL, np.uint8), np.full(n, FILL, np.int32), np.full((V, 4), FILL, np.int32)
    code = lib.hvd_pdq_hash_frames_autocrop_gray_u8(frames.ctypes.data, n, H96, W128, off.ctypes.data, V, 16, 1, hs.ctypes.data,
                                                    q.ctypes.data, rc.ctypes.data)
    return code, hs, q, rc


# Batches end on video boundaries. [5, 0, 4, 3, 1, 4] under 5 frames a batch: {5, 0} (a video exactly at the limit, an empty
# one), {4}, {3, 1} (a run of short videos shares a batch), {4}. A video above the limit is refused (below), so these lengths
# need 5; the second row is the same walk at 4 frames a batch, with empty videos at the end, which upload no frame at all.
AUTOCROP = [([5, 0, 4, 3, 1, 4], 5), ([4, 0, 4, 3, 1, 4, 0, 0], 4)]


@pytest.mark.parametrize("lengths,per_batch", AUTOCROP, ids=["limit5", "limit4"])
def test_autocrop_batches_end_on_video_boundaries(gpu, hvd, oracle, lengths, per_batch):
    frames, off = barred_videos(lengths, 100)
    one = hvd.vpdq.hash_frames_autocrop(frames, off)
    with staging_limit(gpu, per_batch * H96 * W128):
        many = hvd.vpdq.hash_frames_autocrop(frames, off)
    assert same(many, one), (many[2].tolist(), one[2].tolist())
    rule = A.rule_rects(frames, off)
    assert len({tuple(r) for r in rule.tolist()}) >= 5 and (rule != (0, 0, H96, W128)).any(1).sum() >= 3
    assert np.array_equal(one[2], rule)
    assert same(one[:2], A.oracle_cropped(oracle, frames, off, rule))


@pytest.mark.parametrize("lengths", [[5], [5, 0, 4, 3, 1, 4], [4, 2, 5, 1]], ids=str)
def test_autocrop_video_above_the_limit_is_refused_before_anything_is_written(gpu, lengths):
    frames, off = barred_videos(lengths, 200)
    with staging_limit(gpu, 4 * H96 * W128):
        code, hs, q, rc = raw_autocrop(gpu, frames, off)
        msg = gpu.last_error()
    assert code == gpu.HVD_ERR_ARG
    assert f"video {lengths.index(5)} has 5 frames" in msg and "staging limit" in msg, msg
    assert (hs == FILL).all() and (q == FILL).all() and (rc == FILL).all()
    code, hs, q, rc = raw_autocrop(gpu, frames, off)  # the default limit is back
    assert code == gpu.HVD_OK and np.array_equal(rc, A.rule_rects(frames, off))


def test_autocrop_full_rectangles_take_the_plain_kernels_in_every_batch(gpu, hvd, oracle):
    """All-bright frames: every rectangle is the full frame and every batch takes the shortcut to the plain kernels."""
    lengths = [3, 2, 4, 1]
    frames, off = join([np.random.default_rng(300 + v).integers(17, 256, (n, H96, W128), dtype=np.uint8) for v, n in enumerate(lengths)])
    one = hvd.vpdq.hash_frames_autocrop(frames, off)
    with staging_limit(gpu, 4 * H96 * W128):
        many = hvd.vpdq.hash_frames_autocrop(frames, off)
    assert same(many, one) and (one[2] == (0, 0, H96, W128)).all()
    assert same(one[:2], hvd.vpdq.hash_frames(frames)) and same(one[:2], oracle.hash_frames(frames, num_threads=4))
