"""Content-rectangle PDQ on the GPU (run with -m gpu on an MI355X): the rectangles of k_content_rect against
the numpy restatement of the rule, the hashes, qualities and 64x64 planes of the rectangle down-sampler against the oracle's
over the contiguous crops, and the feature end to end. Every comparison is equality."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import autocrop_helpers as A
from conftest import ROOT
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu


# ---- helpers ----

def paint(n, h, w, ch, rect, seed, bar_max=8, lo=40):
    """n frames: bar pixels uniform in [0, bar_max], content uniform in [lo, 255] inside rect = (top, left, hh, ww)."""
    rng = np.random.default_rng(seed)
    shape = (n, h, w) if ch == 1 else (n, h, w, 3)
    fr = rng.integers(0, bar_max + 1, shape, dtype=np.uint8)
    if rect is not None:
        t, l, hh, ww = rect
        fr[:, t:t + hh, l:l + ww] = rng.integers(lo, 256, (n, hh, ww) + shape[3:], dtype=np.uint8)
    return fr


def join(videos):
    off = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(videos)), off


@contextlib.contextmanager
def dct_mode(hvd, mode):
    hvd.vpdq.set_dct_mode(mode)
    try:
        yield
    finally:
        hvd.vpdq.set_dct_mode("strict")


def shifted_frames(gpu, frames, shift):
    """(buffer, device pointer) of the frames copied `shift` bytes behind an aligned allocation."""
    frames = np.ascontiguousarray(frames)
    buf = gpu.DeviceBuffer(frames.nbytes + shift)
    gpu.check(gpu.load().hvd_memcpy_h2d(buf.ptr + shift, frames.ctypes.data, frames.nbytes))
    return buf, buf.ptr + shift


def device_rects(gpu, frames, offsets, level=16, bright=1, shift=0):
    """hvd_dev_content_rects into a sentinel-tailed int32[V][4] buffer."""
    lib = gpu.ensure()
    n, h, w = frames.shape[:3]
    V = len(offsets) - 1
    d_fr, fr_ptr = shifted_frames(gpu, frames, shift)
    bufs = [d_fr, gpu.DeviceBuffer.from_array(offsets), _sentinel_buffer(gpu, 16 * V)]
    try:
        gpu.check(lib.hvd_dev_content_rects(fr_ptr, n, h, w, 3 if frames.ndim == 4 else 1, bufs[1].ptr, V, level, bright,
                                            bufs[2].ptr))
        gpu.check(lib.hvd_dev_sync())
        rects = bufs[2].to_array(np.int32, 4 * V).reshape(V, 4)
        assert _tail_intact(gpu, bufs[2], 16 * V), "rectangle buffer overrun"
    finally:
        for b in bufs:
            b.free()
    return rects


def device_rect_hash(gpu, frames, offsets, rects, shift=0):
    """(planes, hashes, quality) of hvd_dev_pdq_hash_frames_rects on exactly hvd_pdq_rects_scratch_bytes of scratch; every
    output buffer is filled with a sentinel byte and followed by a sentinel tail that must survive."""
    lib = gpu.ensure()
    n, h, w = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    V = len(offsets) - 1
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_pdq_rects_scratch_bytes(n, h, w, ch, C.byref(sb)))
    bufs = []
    try:
        d_fr, fr_ptr = shifted_frames(gpu, frames, shift)
        bufs += [d_fr, gpu.DeviceBuffer.from_array(offsets),
                 gpu.DeviceBuffer.from_array(np.ascontiguousarray(rects, dtype=np.int32))]
        for nbytes in (sb.value, 32 * n, 4 * n):
            bufs.append(_sentinel_buffer(gpu, nbytes))
        d_fr, d_off, d_rc, d_scr, d_h, d_q = bufs
        assert sb.value % 16 == 0 or (h, w) == (64, 64)
        gpu.check(lib.hvd_dev_pdq_hash_frames_rects(fr_ptr, n, h, w, ch, d_off.ptr, V, d_rc.ptr, d_scr.ptr, d_h.ptr, d_q.ptr))
        gpu.check(lib.hvd_dev_sync())
        planes = d_scr.to_array(np.float32, 4096 * n).reshape(n, 64, 64) if sb.value else None
        hashes = d_h.to_array(np.uint8, 32 * n).reshape(n, 32)
        quality = d_q.to_array(np.int32, n)
        assert _tail_intact(gpu, d_scr, sb.value), "scratch overrun"
        assert _tail_intact(gpu, d_h, 32 * n), "hash buffer overrun"
        assert _tail_intact(gpu, d_q, 4 * n), "quality buffer overrun"
    finally:
        for b in bufs:
            b.free()
    return planes, hashes, quality


def check_case(gpu, hvd, oracle, frames, offsets, level=16, bright=1, want_rects=None, modes=("strict", "fma")):
    """Rectangles == the rule (device entry, Python entry, host entry); hashes and qualities of the host entry and of the
    device entry == the oracle's over the contiguous crops, in both DCT modes; planes == the oracle's, bit for bit."""
    rule = A.rule_rects(frames, offsets, level, bright)
    if want_rects is not None:
        assert rule.tolist() == np.asarray(want_rects).tolist(), "the case does not build what it says"
    got = device_rects(gpu, frames, offsets, level, bright)
    assert np.array_equal(got, rule), (got[(got != rule).any(1)][:4], rule[(got != rule).any(1)][:4])
    assert np.array_equal(hvd.vpdq.content_rects(frames, offsets, level, bright), rule)
    wh, wq, wp = A.oracle_cropped(oracle, frames, offsets, rule, planes=True)
    for mode in modes:
        with dct_mode(hvd, mode):
            if mode == "fma":
                wh, wq = A.oracle_cropped(oracle, frames, offsets, rule, fma=True)
            h, q, r = hvd.vpdq.hash_frames_autocrop(frames, offsets, level, bright)
            assert np.array_equal(r, rule), mode
            assert np.array_equal(q, wq), (mode, np.flatnonzero(q != wq)[:8])
            assert np.array_equal(h, wh), (mode, np.flatnonzero((h != wh).any(1))[:8])
            planes, dh, dq = device_rect_hash(gpu, frames, offsets, rule)
            if planes is not None:  # (64x64 gray has no plane: the u8 frame is the hash kernel's input)
                bad = np.flatnonzero((planes.view(np.uint32) != wp.view(np.uint32)).any(axis=(1, 2)))
                assert bad.size == 0, (mode, f"{bad.size} planes differ, first frame {bad[0]}")
            assert np.array_equal(dq, wq) and np.array_equal(dh, wh), mode
    return rule


# ---- 5 + 6. rectangles == the rule, hashes / qualities / planes == the oracle's over the crops ----

def test_the_four_layouts(gpu, hvd, oracle):
    rng = np.random.default_rng(5)
    vids, rects = [], []
    for b, ax in A.LAYOUTS:
        fr, rc = A.barred(3, b, ax, rng, nf=2)
        vids.append(fr)
        rects.append(rc)
    frames, off = join(vids)
    check_case(gpu, hvd, oracle, frames, off, want_rects=rects)


def test_bars_on_all_four_sides_odd_origin(gpu, hvd, oracle):
    frames, off = join([paint(3, 512, 512, 3, (37, 51, 300, 401), 1), paint(2, 512, 512, 3, (1, 3, 510, 507), 2)])
    check_case(gpu, hvd, oracle, frames, off, want_rects=[(37, 51, 300, 401), (1, 3, 510, 507)])


def test_no_bars_all_dark_and_narrow_content(gpu, hvd, oracle):
    """No bars; an all-dark video (full frame); only bright frames narrower than 64 on one axis (that axis keeps its full
    extent, the other is cropped)."""
    h, w = 256, 320
    frames, off = join([paint(2, h, w, 3, (0, 0, h, w), 3), paint(2, h, w, 3, None, 4), paint(2, h, w, 3, (10, 100, 200, 40), 5),
                        paint(2, h, w, 3, (100, 16, 63, 288), 6)])
    check_case(gpu, hvd, oracle, frames, off, want_rects=[(0, 0, h, w), (0, 0, h, w), (10, 0, 200, w), (0, 16, h, 288)])


def test_content_of_exactly_64x64(gpu, hvd, oracle):
    """A 64 x 64 rectangle inside a larger frame hashes as a 64 x 64 frame does: from its luma, unfiltered."""
    for ch in (1, 3):
        frames, off = join([paint(2, 200, 240, ch, (30, 41, 64, 64), 12), paint(2, 200, 240, ch, (3, 5, 64, 65), 13),
                            paint(1, 200, 240, ch, (136, 176, 64, 64), 14)])
        check_case(gpu, hvd, oracle, frames, off, want_rects=[(30, 41, 64, 64), (3, 5, 64, 65), (136, 176, 64, 64)])


def test_dark_frame_in_the_middle_keeps_the_video_box(gpu, hvd, oracle):
    v = paint(5, 300, 400, 3, (40, 0, 220, 400), 7)
    v[2] = paint(1, 300, 400, 3, None, 8)[0]
    w = paint(3, 300, 400, 3, (40, 0, 220, 400), 9)   # frames with different boxes: the video's is their bounding box
    w[1] = paint(1, 300, 400, 3, (20, 30, 100, 100), 10)[0]
    frames, off = join([v, w])
    check_case(gpu, hvd, oracle, frames, off, want_rects=[(40, 0, 220, 400), (20, 0, 240, 400)])


def test_speckles_in_the_bars_and_min_bright(gpu, hvd, oracle):
    v = paint(3, 240, 320, 1, (50, 40, 140, 240), 11)
    v[1, 5, [3, 100, 319]] = 200     # three speckles in one bar row, in three bar columns
    frames, off = join([v])
    check_case(gpu, hvd, oracle, frames, off, bright=1, want_rects=[(5, 3, 185, 317)])
    check_case(gpu, hvd, oracle, frames, off, bright=3, want_rects=[(5, 40, 185, 240)])  # the row counts 3
    check_case(gpu, hvd, oracle, frames, off, bright=4, want_rects=[(50, 40, 140, 240)])


@pytest.mark.parametrize("ch", [1, 3])
def test_black_level_is_strictly_greater(gpu, hvd, oracle, ch):
    shape = (2, 200, 208) + ((3,) if ch == 3 else ())
    fr = np.full(shape, 8, np.uint8)
    fr[:, 30:170, 16:200] = 40
    off = np.array([0, 2], dtype=np.int64)
    inner, full = [(30, 16, 140, 184)], [(0, 0, 200, 208)]
    check_case(gpu, hvd, oracle, fr, off, level=8, want_rects=inner)
    check_case(gpu, hvd, oracle, fr, off, level=7, want_rects=full)
    check_case(gpu, hvd, oracle, fr, off, level=39, want_rects=inner)
    check_case(gpu, hvd, oracle, fr, off, level=40, want_rects=full)
    check_case(gpu, hvd, oracle, fr, off, level=0, want_rects=full)
    check_case(gpu, hvd, oracle, fr, off, level=254, want_rects=full)


def test_rgb_pixel_bright_in_one_channel_only(gpu, hvd, oracle):
    vids, rects = [], []
    for c in range(3):
        fr = paint(2, 160, 192, 3, None, 20 + c)
        t, l = 11 + c, 7 + 5 * c
        fr[:, t:t + 90, l:l + 100, c] = np.random.default_rng(c).integers(17, 256, (2, 90, 100), dtype=np.uint8)
        vids.append(fr)
        rects.append((t, l, 90, 100))
    frames, off = join(vids)
    check_case(gpu, hvd, oracle, frames, off, want_rects=rects)


def test_zero_frame_video_between_two_others(gpu, hvd, oracle):
    a, b = paint(3, 128, 160, 3, (20, 0, 88, 160), 30), paint(2, 128, 160, 3, (0, 40, 128, 80), 31)
    frames = np.concatenate([a, b])
    off = np.array([0, 0, 3, 3, 3, 5, 5], dtype=np.int64)
    full = (0, 0, 128, 160)
    check_case(gpu, hvd, oracle, frames, off, want_rects=[full, (20, 0, 88, 160), full, full, (0, 40, 128, 80), full])


GEOMETRIES = [(64, 64, None), (360, 640, (45, 0, 270, 640)), (480, 853, (0, 107, 480, 639)), (512, 512, (64, 0, 384, 512)),
              (1080, 1920, (140, 0, 800, 1920))]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("h,w,rect", GEOMETRIES, ids=[f"{h}x{w}" for h, w, _ in GEOMETRIES])
def test_frame_geometries(gpu, hvd, oracle, h, w, rect, ch):
    """64x64 (every rectangle is full by the rule: content 40 wide keeps the full frame), letterbox / pillarbox at video sizes;
    480x853: rows that are not 16-byte aligned (the byte-load form of k_content_rect)."""
    if rect is None:
        frames, off = join([paint(3, h, w, ch, (8, 12, 40, 40), 40), paint(2, h, w, ch, (0, 0, 64, 64), 41)])
        check_case(gpu, hvd, oracle, frames, off, want_rects=[(0, 0, 64, 64)] * 2)
    else:
        t, l, hh, ww = rect
        frames, off = join([paint(2, h, w, ch, rect, 42), paint(1, h, w, ch, (0, 0, h, w), 43),
                            paint(2, h, w, ch, (t + 1, l + 3, hh - 2, ww - 7), 44)])
        check_case(gpu, hvd, oracle, frames, off, want_rects=[rect, (0, 0, h, w), (t + 1, l + 3, hh - 2, ww - 7)])


@pytest.mark.parametrize("ch", [1, 3])
def test_odd_geometry_with_an_odd_frame_count(gpu, hvd, oracle, ch):
    """h * w odd and n odd: the workspace ends on an 8-byte boundary only, the frame -> rectangle table behind it must still
    start on a 16-byte one (hvd_pdq_rects_scratch_bytes rounds)."""
    frames, off = join([paint(2, 81, 85, ch, (3, 5, 70, 77), 45), paint(1, 81, 85, ch, (0, 0, 81, 85), 46)])
    sb, plain = C.c_size_t(0), C.c_size_t(0)
    lib = gpu.ensure()
    gpu.check(lib.hvd_pdq_rects_scratch_bytes(3, 81, 85, ch, C.byref(sb)))
    gpu.check(lib.hvd_pdq_scratch_bytes(3, 81, 85, ch, C.byref(plain)))
    assert plain.value % 16 == 8 and sb.value == plain.value + 8 + 16 * 3
    check_case(gpu, hvd, oracle, frames, off, want_rects=[(3, 5, 70, 77), (0, 0, 81, 85)])


@pytest.mark.parametrize("ch", [1, 3])
def test_frames_at_an_odd_address(gpu, hvd, oracle, ch):
    """A width that is a multiple of 16 but a frame base that is not 16-byte aligned: k_content_rect's byte-load form; the
    down-sampler reads bytes anyway."""
    rects = [(9, 16, 100, 112), (0, 0, 128, 160)]
    frames, off = join([paint(2, 128, 160, ch, rects[0], 47), paint(2, 128, 160, ch, rects[1], 48)])
    rule = A.rule_rects(frames, off)
    assert rule.tolist() == [list(r) for r in rects]
    wh, wq, wp = A.oracle_cropped(oracle, frames, off, rule, planes=True)
    for shift in (1, 8, 13):
        assert np.array_equal(device_rects(gpu, frames, off, shift=shift), rule), shift
        planes, h, q = device_rect_hash(gpu, frames, off, rule, shift=shift)
        assert np.array_equal(planes.view(np.uint32), wp.view(np.uint32)), shift
        assert np.array_equal(h, wh) and np.array_equal(q, wq), shift


@pytest.mark.parametrize("ch,w", [(1, 2064), (3, 4096), (1, 4095)])
def test_rows_wider_than_2048_pixels(gpu, hvd, oracle, ch, w):
    """More than 128 units of 16 pixels per row: all 256 lanes of k_content_rect's workgroup share one row (P = 256)."""
    h = 70
    frames, off = join([paint(2, h, w, ch, (2, 33, 65, w - 100), 49), paint(1, h, w, ch, (0, 0, h, w), 50)])
    check_case(gpu, hvd, oracle, frames, off, want_rects=[(2, 33, 65, w - 100), (0, 0, h, w)])


def test_jarosz_window_edges_and_odd_origins(gpu, hvd, oracle):
    """Rectangle sides on both edges of a Jarosz window (128k and 128k + 1), origins that are no multiples of 4 (RGB row
    starts not 16-byte aligned), several geometries in one call."""
    h, w = 600, 700
    rects = [(3, 5, 256, 512), (1, 7, 257, 513), (9, 2, 384, 640), (13, 11, 385, 641), (101, 33, 128, 129), (2, 1, 129, 128),
             (0, 0, 512, 513), (88, 60, 512, 640)]
    vids = [paint(2, h, w, 3, rc, 50 + i) for i, rc in enumerate(rects)]
    frames, off = join(vids)
    check_case(gpu, hvd, oracle, frames, off, want_rects=rects)
    gray, off = join([paint(2, h, w, 1, rc, 60 + i) for i, rc in enumerate(rects[:4])])
    check_case(gpu, hvd, oracle, gray, off, want_rects=rects[:4])


def test_caller_rectangles_need_no_bars(gpu, hvd, oracle):
    """hvd_dev_pdq_hash_frames_rects takes any rectangle inside the frame: unbarred content, the caller's own geometry."""
    fr = hvd.synth.frames_rgb(6, seed=70, h=300, w=420)
    off = np.array([0, 2, 4, 6], dtype=np.int64)
    rects = np.array([(17, 23, 129, 257), (0, 0, 300, 420), (236, 356, 64, 64)], dtype=np.int32)
    wh, wq, wp = A.oracle_cropped(oracle, fr, off, rects, planes=True)
    planes, h, q = device_rect_hash(gpu, fr, off, rects)
    assert np.array_equal(planes.view(np.uint32), wp.view(np.uint32))
    assert np.array_equal(h, wh) and np.array_equal(q, wq)
    # a record that is not inside the frame is taken as the full frame (never an access out of bounds)
    bad = np.array([(250, 0, 129, 420), (0, 0, 300, 421), (-1, 0, 63, 64)], dtype=np.int32)
    wh, wq = oracle.hash_frames(fr, num_threads=4)
    _, h, q = device_rect_hash(gpu, fr, off, bad)
    assert np.array_equal(h, wh) and np.array_equal(q, wq)


@pytest.fixture(scope="module")
def big_batch():
    """3 100 videos of mixed layouts, 0..4 frames each (one of 300), 96x112 RGB: more than 1024 frames, so the slab border is
    crossed, and many frames fold into one video's box at once."""
    h, w = 96, 112
    layouts = [(0, 0, h, w), (12, 0, 72, w), (0, 16, h, 80), (7, 9, 70, 90), None, (10, 20, 30, 80)]
    rng = np.random.default_rng(80)
    vids = []
    for v in range(3100):
        n = 300 if v == 1500 else int(rng.integers(0, 5))
        fr = paint(n, h, w, 3, layouts[v % len(layouts)], 1000 + v)
        if n > 1 and v % 7 == 0:
            fr[0] = paint(1, h, w, 3, None, 5000 + v)[0]  # a dark frame
        vids.append(fr)
    return join(vids)


def test_batch_of_3100_videos_crosses_slabs(gpu, hvd, oracle, big_batch):
    frames, off = big_batch
    assert len(frames) > 3 * 1024 and len(off) - 1 >= 3000
    rule = check_case(gpu, hvd, oracle, frames, off)
    assert len({tuple(r) for r in rule.tolist()}) >= 5


# ---- 7. full rectangles: the autocrop entry == the plain entry ----

@pytest.mark.parametrize("n", [703, 704])
def test_full_rectangles_512_fused_path(gpu, hvd, n):
    fr = np.random.default_rng(n).integers(17, 256, (n, 512, 512, 3), dtype=np.uint8)
    off = np.arange(0, n + 1, 64, dtype=np.int64)
    off = np.append(off, n) if off[-1] != n else off
    h, q, r = hvd.vpdq.hash_frames_autocrop(fr, off)
    assert (r == (0, 0, 512, 512)).all()
    wh, wq = hvd.vpdq.hash_frames(fr)
    assert np.array_equal(h, wh) and np.array_equal(q, wq)


def test_full_rectangles_64_gray_and_480x853(gpu, hvd):
    for fr in (hvd.synth.frames_gray(500, seed=90), np.random.default_rng(91).integers(17, 256, (9, 480, 853, 3), dtype=np.uint8)):
        h, q, r = hvd.vpdq.hash_frames_autocrop(fr, [0, 4, len(fr)])
        assert (r == (0, 0) + fr.shape[1:3]).all()
        wh, wq = hvd.vpdq.hash_frames(fr)
        assert np.array_equal(h, wh) and np.array_equal(q, wq)


# ---- 8. error codes, n = 0 ----

def test_error_codes_and_empty_calls(gpu, hvd):
    lib = gpu.ensure()
    fr = paint(4, 128, 128, 3, (10, 10, 100, 100), 95)
    off = np.array([0, 2, 4], dtype=np.int64)
    d_fr, d_off, d_rc = gpu.DeviceBuffer.from_array(fr), gpu.DeviceBuffer.from_array(off), gpu.DeviceBuffer(64)
    d_h, d_q, d_s = gpu.DeviceBuffer(128), gpu.DeviceBuffer(16), gpu.DeviceBuffer(1 << 20)
    sb = C.c_size_t(0)
    ARG = gpu.HVD_ERR_ARG
    try:
        for h, w, ch in ((63, 128, 3), (128, 4097, 3), (128, 128, 2), (128, 128, 0)):
            assert lib.hvd_dev_content_rects(d_fr.ptr, 4, h, w, ch, d_off.ptr, 2, 16, 1, d_rc.ptr) == ARG
            assert lib.hvd_pdq_rects_scratch_bytes(4, h, w, ch, C.byref(sb)) == ARG
            assert lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, 4, h, w, ch, d_off.ptr, 2, d_rc.ptr, d_s.ptr, d_h.ptr, d_q.ptr) == ARG
        assert "geometry" in gpu.last_error()
        assert lib.hvd_dev_content_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, 255, 1, d_rc.ptr) == ARG
        assert lib.hvd_dev_content_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, 16, 0, d_rc.ptr) == ARG
        assert lib.hvd_dev_content_rects(d_fr.ptr, 4, 128, 128, 3, None, 2, 16, 1, d_rc.ptr) == ARG
        assert lib.hvd_dev_content_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 0, 16, 1, d_rc.ptr) == ARG  # frames in no video
        gpu.check(lib.hvd_dev_content_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, 16, 1, d_rc.ptr))
        assert lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, d_rc.ptr, None, d_h.ptr, d_q.ptr) == ARG
        assert "scratch" in gpu.last_error()
        assert lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, None, d_s.ptr, d_h.ptr, d_q.ptr) == ARG
        # records are accessed as 16-byte words: a misaligned rectangle buffer or scratch is refused
        assert lib.hvd_dev_content_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, 16, 1, d_rc.ptr + 4) == ARG
        assert "aligned" in gpu.last_error()
        assert lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, d_rc.ptr + 8, d_s.ptr, d_h.ptr, d_q.ptr) == ARG
        assert lib.hvd_dev_pdq_hash_frames_rects(d_fr.ptr, 4, 128, 128, 3, d_off.ptr, 2, d_rc.ptr, d_s.ptr + 4, d_h.ptr, d_q.ptr) == ARG
        # n = 0 / V = 0
        gpu.check(lib.hvd_dev_content_rects(None, 0, 128, 128, 3, None, 0, 16, 1, None))
        gpu.check(lib.hvd_dev_pdq_hash_frames_rects(None, 0, 128, 128, 3, None, 0, None, None, None, None))
        gpu.check(lib.hvd_pdq_rects_scratch_bytes(0, 128, 128, 3, C.byref(sb)))
        gpu.check(lib.hvd_pdq_rects_scratch_bytes(5, 64, 64, 1, C.byref(sb)))
        assert sb.value == 0
        gpu.check(lib.hvd_dev_sync())
        # host entry: offsets are validated
        hs, q, rc = np.zeros((4, 32), np.uint8), np.zeros(4, np.int32), np.zeros((2, 4), np.int32)
        fn = lib.hvd_pdq_hash_frames_autocrop_rgb24_u8
        for bad in ([1, 2, 4], [0, 3, 2], [0, 2, 5]):
            o = np.array(bad, dtype=np.int64)
            assert fn(fr.ctypes.data, 4, 128, 128, o.ctypes.data, 2, 16, 1, hs.ctypes.data, q.ctypes.data, rc.ctypes.data) == ARG
            assert "offsets" in gpu.last_error()
        assert fn(fr.ctypes.data, 4, 128, 63, off.ctypes.data, 2, 16, 1, hs.ctypes.data, q.ctypes.data, rc.ctypes.data) == ARG
        assert fn(fr.ctypes.data, 4, 128, 128, off.ctypes.data, 2, 300, 1, hs.ctypes.data, q.ctypes.data, rc.ctypes.data) == ARG
        gpu.check(fn(None, 0, 128, 128, None, 0, 16, 1, None, None, None))
        # only empty videos: full frames, nothing hashed
        o = np.zeros(3, dtype=np.int64)
        gpu.check(fn(None, 0, 128, 128, o.ctypes.data, 2, 16, 1, None, None, rc.ctypes.data))
        assert rc.tolist() == [[0, 0, 128, 128]] * 2
    finally:
        for b in (d_fr, d_off, d_rc, d_h, d_q, d_s):
            b.free()
    h0, q0, r0 = hvd.vpdq.hash_frames_autocrop(np.zeros((0, 128, 128, 3), np.uint8))
    assert h0.shape == (0, 32) and q0.shape == (0,) and r0.tolist() == [[0, 0, 128, 128]]


def test_a_video_beyond_the_staging_limit_is_rejected_not_split(gpu):
    """One video of more frames than fit 1 GiB of staging: HVD_ERR_ARG with a message that says so (the argument check
    comes before any frame is read, so the frame pointer can stay a small buffer)."""
    lib = gpu.ensure()
    h = w = 4096
    n = (1 << 30) // (h * w * 3) + 1
    off = np.array([0, n], dtype=np.int64)
    fr = np.zeros(16, np.uint8)
    hs, q, rc = np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.zeros((1, 4), np.int32)
    assert lib.hvd_pdq_hash_frames_autocrop_rgb24_u8(fr.ctypes.data, n, h, w, off.ctypes.data, 1, 16, 1, hs.ctypes.data,
                                                     q.ctypes.data, rc.ctypes.data) == gpu.HVD_ERR_ARG
    assert "staging limit" in gpu.last_error()


# ---- 9. end to end ----

@pytest.fixture(scope="module")
def library(oracle):
    frames, offsets, rects, groups = A.library_30()
    cropped, _ = A.oracle_cropped(oracle, frames, offsets, rects)
    want = oracle.match_videos(cropped, offsets, A.FRAME_TOLERANCE)
    assert len(want) == 60
    return frames, offsets, rects, groups, want


def test_library_of_30_videos_end_to_end(gpu, hvd, oracle, library):
    frames, offsets, rects, groups, want = library
    h, q, r = hvd.vpdq.hash_frames_autocrop(frames, offsets)
    assert np.array_equal(r, rects) and q.min() >= 31
    recs = hvd.search.match_videos(h, offsets, A.FRAME_TOLERANCE)
    assert recs.dtype == want.dtype and np.array_equal(recs, want)
    videos = [frames[offsets[v]:offsets[v + 1]] for v in range(30)]
    phashes = hvd.pipeline.hash_videos(videos, autocrop=True)
    assert [p.bytes for p in phashes] == [h[offsets[v]:offsets[v + 1]].tobytes() for v in range(30)]
    assert hvd.search.find_potential_duplicates(phashes, threshold=50) == A.expected_pairs(groups)
    # Vpdq.computeHash(autocrop=...) is the same video hash
    from hvd_amd.vpdqpy import Vpdq
    for v in (0, 1, 3):
        assert Vpdq.computeHash(videos[v], autocrop=True).bytes == phashes[v].bytes
        assert Vpdq.computeHash(videos[v], autocrop={"black_level": 16, "min_bright": 1}).bytes == phashes[v].bytes
    assert Vpdq.computeHash(videos[1]).bytes == hvd.pipeline.hash_videos(videos[1:2])[0].bytes != phashes[1].bytes
    # without the rectangle nothing is found
    plain = hvd.pipeline.hash_videos(videos)
    assert hvd.search.find_potential_duplicates(plain, threshold=50) == []


# ---- 10. the chained pipeline ----

def test_pipeline_on_device_with_autocrop(gpu, hvd, oracle, library):
    frames, offsets, rects, groups, want = library
    d_fr = gpu.DeviceBuffer.from_array(frames)
    try:
        tm = {}
        pairs, recs, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop=True, timings=tm)
        assert [tuple(p) for p in pairs.tolist()] == A.expected_pairs(groups)
        assert np.array_equal(recs, want)
        assert tm["rects_ms"] > 0 and tm["hash_ms"] > 0 and "search_ms" in tm
        pairs2, recs2, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop={"black_level": 9, "min_bright": 2})
        assert np.array_equal(pairs2, pairs) and np.array_equal(recs2, recs)
        # autocrop=None: today's result
        tm0 = {}
        p0, r0, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop=None, timings=tm0)
        p1, r1, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3)
        ph, pq = oracle.hash_frames(frames, num_threads=8)
        assert pq.min() >= 31
        assert np.array_equal(r0, oracle.match_videos(ph, offsets, A.FRAME_TOLERANCE)) and len(p0) == 0
        assert np.array_equal(r0, r1) and np.array_equal(p0, p1) and "rects_ms" not in tm0
        pi, ri = hvd.pipeline.dedupe_frames_in_process(lambda rank, world: d_fr.ptr, offsets, 512, 512, 3, autocrop=True)
        assert np.array_equal(pi, pairs) and np.array_equal(ri, recs)
    finally:
        d_fr.free()


def test_host_entry_under_a_device_group(gpu):
    """HVD_DEVICES=0,0 (one GPU listed twice: two contexts): the host entry returns the same bytes as on one context."""
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"}
    env["HVD_DEVICES"] = "0,0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "autocrop_group_check.py")], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert r.returncode == 0 and "AUTOCROP_GROUP_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
