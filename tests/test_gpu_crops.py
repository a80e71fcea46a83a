"""Crop-ladder PDQ on the device: hvd_dev_pdq_hash_frames_crops and its host-buffer forms against
oracle.hash_frames on the contiguous numpy crop, byte for byte, in both DCT modes, at the shapes where k_down_crops, its 64 x 64
branch, the slabs and the generic passes can go wrong."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import crops_helpers as H

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def dct_mode(hvd, mode):
    hvd.vpdq.set_dct_mode(mode)
    try:
        yield
    finally:
        hvd.vpdq.set_dct_mode("strict")


def noise(seed, n, h, w, ch):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if ch == 1 else (n, h, w, 3), dtype=np.uint8)


FILL = 0xA5  # what every output buffer holds before a call: a slot the library does not write shows


def device_crops(gpu, frames, rects, with_crop_quality=True):
    """hvd_dev_pdq_hash_frames_crops on an exactly sized device copy of the frames, the outputs pre-filled with FILL
    -> (uint8[n,8,32], int32[n], int32[n,8])."""
    lib = gpu.load()
    frames = np.ascontiguousarray(frames)
    rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    n, h, w = frames.shape[:3]
    K = rects.shape[0]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_pdq_crops_scratch_bytes(n, h, w, K, C.byref(sb)))
    filled = lambda nbytes: gpu.DeviceBuffer.from_array(np.full(max(nbytes, 1), FILL, np.uint8))
    bufs = [gpu.DeviceBuffer.from_array(frames) if n else gpu.DeviceBuffer(1), filled(sb.value), filled(256 * n), filled(4 * n),
            filled(32 * n)]
    d_fr, d_s, d_h, d_q, d_cq = bufs
    try:
        gpu.check(lib.hvd_dev_pdq_hash_frames_crops(d_fr.ptr if n else None, n, h, w, 1 if frames.ndim == 3 else 3, rects.ctypes.data,
                                                    K, d_s.ptr, d_h.ptr, d_q.ptr, d_cq.ptr if with_crop_quality else None))
        out = (d_h.to_array(np.uint8, 256 * n).reshape(n, 8, 32), d_q.to_array(np.int32, n), d_cq.to_array(np.int32, 8 * n).reshape(n, 8))
        gpu.check(lib.hvd_dev_sync())
    finally:
        for b in bufs:
            b.free()
    return out


def host_crops(gpu, frames, rects):
    """The host-buffer entry on raw output buffers pre-filled with FILL -> all 8 slots: (uint8[n,8,32], int32[n], int32[n,8])."""
    lib = gpu.load()
    frames = np.ascontiguousarray(frames)
    rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    n, h, w = frames.shape[:3]
    fn = lib.hvd_pdq_hash_frames_crops_gray_u8 if frames.ndim == 3 else lib.hvd_pdq_hash_frames_crops_rgb24_u8
    h8, q, cq = np.full((n, 8, 32), FILL, np.uint8), np.full(n, FILL, np.int32), np.full((n, 8), FILL, np.int32)
    gpu.check(fn(frames.ctypes.data, n, h, w, rects.ctypes.data, rects.shape[0], h8.ctypes.data, q.ctypes.data, cq.ctypes.data))
    return h8, q, cq


def check_against_oracle(hvd, gpu, oracle, frames, rects, modes=("strict", "fma"), distinct=None):
    """distinct: the frames are frames[:distinct] repeated; the oracle hashes those and its answers are repeated likewise."""
    rects = np.asarray(rects, dtype=np.int32).reshape(-1, 4)
    K = rects.shape[0]
    n = frames.shape[0]
    for mode in modes:
        want_h, want_q = H.oracle_crops(oracle, frames if distinct is None else frames[:distinct], rects, fma=mode == "fma")
        if distinct is not None:
            idx = np.arange(n) % distinct
            want_h, want_q = want_h[idx], want_q[idx]
        with dct_mode(hvd, mode):
            h8, q, cq = device_crops(gpu, frames, rects)
            plain_h, plain_q = hvd.vpdq.hash_frames(frames)
            raw_h, raw_q, raw_cq = host_crops(gpu, frames, rects)
            host_h, host_q, host_cq, names = hvd.vpdq.hash_frames_crops(frames, tuple(map(tuple, rects.tolist())))
        bad = np.argwhere((h8[:, :K + 1] != want_h).any(axis=2))
        assert bad.size == 0, (mode, "hashes differ from the oracle at (frame, slot)", bad[:6].tolist())
        assert np.array_equal(cq[:, :K + 1], want_q), (mode, np.argwhere(cq[:, :K + 1] != want_q)[:6].tolist())
        assert not h8[:, K + 1:].any() and not cq[:, K + 1:].any(), "slots above K must be written, as zero"
        assert np.array_equal(q, want_q[:, 0])
        assert np.array_equal(h8[:, 0], plain_h) and np.array_equal(q, plain_q), "slot 0 is vpdq.hash_frames"
        # the host-buffer entries: all 8 raw slots are the device entry's, the Python form returns the first K + 1
        assert np.array_equal(raw_h, h8) and np.array_equal(raw_q, q) and np.array_equal(raw_cq, cq)
        assert np.array_equal(host_h, h8[:, :K + 1]) and np.array_equal(host_q, q) and np.array_equal(host_cq, cq[:, :K + 1])
        assert len(names) == K and host_h.shape == (n, K + 1, 32)


def test_aspect_ladder_on_512_rgb(hvd, gpu, oracle):
    frames = noise(1, 5, 512, 512, 3)
    _, rects = hvd.vpdq.crop_ladder(512, 512, "aspect")
    assert np.array_equal(rects, H.ladder(512, 512, "aspect")[1])
    check_against_oracle(hvd, gpu, oracle, frames, rects)


def test_landscape_ladder_on_512_gray(hvd, gpu, oracle):
    """At exactly 512 x 512 the full frame is hashed by the plain front-end and the loop starts at the first crop."""
    check_against_oracle(hvd, gpu, oracle, noise(22, 2, 512, 512, 1), hvd.vpdq.crop_ladder(512, 512, "landscape")[1])
    check_against_oracle(hvd, gpu, oracle, noise(23, 2, 512, 512, 3), [(448, 448, 64, 64)])


@pytest.mark.parametrize("n", [1100, 3100])
def test_many_512_frames_take_the_wave_front_end_for_the_full_frame(hvd, gpu, oracle, n):
    """From 704 frames of 512 x 512 on the full frame goes through k_down512w, whose workspace lies in the crops' scratch, in
    passes of 3 072 frames, next to the loop's slabs of 1 024: 1 100 frames cross a slab, 3 100 a pass as well. 20 distinct
    frames, repeated (20 divides neither 1 024 nor 3 072, so a frame shifted by a slab would show)."""
    frames = np.ascontiguousarray(np.tile(noise(24, 20, 512, 512, 1), (n // 20, 1, 1)))
    check_against_oracle(hvd, gpu, oracle, frames, [(448, 448, 64, 64), (0, 112, 512, 288)], distinct=20)


def test_grid_stride_loop_past_256_workgroups(hvd, gpu, oracle):
    check_against_oracle(hvd, gpu, oracle, noise(2, 300, 96, 80, 1), [(3, 5, 70, 66), (16, 0, 64, 80)])


def test_more_frames_than_a_slab(hvd, gpu, oracle):
    check_against_oracle(hvd, gpu, oracle, noise(3, 1030, 64, 72, 1), [(0, 5, 64, 65)])


def test_one_frame_and_none(hvd, gpu, oracle):
    check_against_oracle(hvd, gpu, oracle, noise(4, 1, 90, 130, 3), [(10, 20, 70, 100)])
    h8, q, cq = device_crops(gpu, np.zeros((0, 90, 130), np.uint8), [(10, 20, 70, 100)])
    assert h8.shape == (0, 8, 32) and q.shape == (0,)
    got = hvd.vpdq.hash_frames_crops(np.zeros((0, 90, 256, 3), np.uint8), "landscape")
    assert got[0].shape == (0, 4, 32) and got[1].shape == (0,) and got[2].shape == (0, 4) and got[3] == H.SETS["landscape"]


@pytest.mark.parametrize("ch", [1, 3])
def test_sides_around_every_window_change(hvd, gpu, oracle, ch):
    """The box filter's window is ceil(side / 128): 128 / 129, 256 / 257, 384 / 385 on each axis."""
    frames = noise(5 + ch, 2, 390, 388, ch)
    sides = (128, 129, 256, 257, 384, 385)
    check_against_oracle(hvd, gpu, oracle, frames, [(k, 3 - k % 4, 100 + k, s) for k, s in enumerate(sides)])
    check_against_oracle(hvd, gpu, oracle, frames, [(5 - k, 2 * k, s, 99 + k) for k, s in enumerate(sides)])


def test_crops_of_64(hvd, gpu, oracle):
    """64 x 64 is the crop's unfiltered luma; 64 x w and h x 64 are filtered along one axis with window 1."""
    for ch in (1, 3):
        check_against_oracle(hvd, gpu, oracle, noise(8 + ch, 3, 100, 120, ch), [(5, 7, 64, 64), (36, 0, 64, 120), (0, 56, 100, 64)])
    check_against_oracle(hvd, gpu, oracle, noise(12, 3, 64, 64, 1), [(0, 0, 64, 64)])
    check_against_oracle(hvd, gpu, oracle, noise(13, 2, 64, 64, 3), [(0, 0, 64, 64), (0, 0, 64, 64)])


@pytest.mark.parametrize("ch", [1, 3])
def test_unaligned_left_edges_and_the_last_pixel_of_the_buffer(hvd, gpu, oracle, ch):
    """left in {1, 2, 3}: the row's first byte at every offset inside its 32-bit word; the last crop ends in the bottom-right
    pixel of the last frame, whose clamped tail loads must stay inside the (exactly sized) buffer."""
    frames = noise(14 + ch, 3, 80, 101, ch)
    check_against_oracle(hvd, gpu, oracle, frames, [(0, 1, 70, 90), (2, 2, 75, 97), (4, 3, 64, 65), (16, 34, 64, 67)])


def test_full_frame_as_a_crop_and_a_duplicate(hvd, gpu, oracle):
    frames = noise(17, 4, 200, 300, 3)
    check_against_oracle(hvd, gpu, oracle, frames, [(0, 0, 200, 300), (20, 30, 150, 200), (20, 30, 150, 200)])


def test_one_crop_and_seven(hvd, gpu, oracle):
    frames = noise(18, 3, 150, 140, 1)
    check_against_oracle(hvd, gpu, oracle, frames, [(1, 1, 149, 139)])
    check_against_oracle(hvd, gpu, oracle, frames, [(k, 2 * k, 64 + 10 * k, 126 - 9 * k) for k in range(7)])
    lib = gpu.load()
    assert lib.hvd_dev_pdq_hash_frames_crops(None, 0, 150, 140, 1, np.zeros((8, 4), np.int32).ctypes.data, 8, None, None, None,
                                             None) == gpu.HVD_ERR_ARG


def test_frames_wider_than_512_take_the_generic_passes(hvd, gpu, oracle):
    frames = noise(19, 2, 100, 520, 1)
    check_against_oracle(hvd, gpu, oracle, frames, [(0, 4, 100, 516), (36, 456, 64, 64), (3, 1, 90, 300)])


def test_crop_quality_is_optional(hvd, gpu):
    frames = noise(20, 3, 96, 80, 3)
    rects = [(3, 5, 70, 66)]
    a = device_crops(gpu, frames, rects)
    b = device_crops(gpu, frames, rects, with_crop_quality=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (b[2].view(np.uint8) == FILL).all(), "a NULL d_crop_quality: nothing of that kind is written anywhere"


def test_null_pointers_and_alignment_are_argument_errors(hvd, gpu):
    lib = gpu.load()
    rects = np.array([[3, 5, 70, 66]], np.int32)
    buf = gpu.DeviceBuffer(1 << 20)
    try:
        args = lambda fr, s, h, q: (fr, 1, 96, 80, 1, rects.ctypes.data, 1, s, h, q, None)
        p = buf.ptr
        assert lib.hvd_dev_pdq_hash_frames_crops(*args(None, p, p, p)) == gpu.HVD_ERR_ARG
        assert lib.hvd_dev_pdq_hash_frames_crops(*args(p, None, p, p)) == gpu.HVD_ERR_ARG
        assert lib.hvd_dev_pdq_hash_frames_crops(*args(p, p + 8, p, p)) == gpu.HVD_ERR_ARG
        assert lib.hvd_dev_pdq_hash_frames_crops(*args(p, p, p + 2, p)) == gpu.HVD_ERR_ARG
        gpu.check(lib.hvd_dev_sync())
    finally:
        buf.free()


def test_computeCroppedHashes(hvd, gpu, oracle):
    frames = noise(21, 6, 128, 256, 3)
    frames[2] = 7  # a flat frame: quality 0, dropped from every variant
    got = hvd.Vpdq.computeCroppedHashes(frames, "landscape")
    names, rects = H.ladder(128, 256, "landscape")
    want_h, want_q = H.oracle_crops(oracle, frames, rects)
    keep = want_q[:, 0] >= 31
    assert not keep[2] and keep.sum() == 5
    assert list(got) == ["identity"] + list(names)
    for k, name in enumerate(got):
        assert got[name].bytes == want_h[keep][:, k].tobytes(), name
    assert got["identity"] == hvd.Vpdq.computeHash(frames)
