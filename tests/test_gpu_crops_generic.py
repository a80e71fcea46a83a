"""Crop-ladder PDQ on frames with a side above 512: what csrc/k_crops.hip puts around the generic rectangle chain
-- k_crops_table's one-video CSR and rectangle list, one launch_pdq_downsample_rects per rectangle, rectangle-major planes,
k_crops_scatter with sf = 1 and sk = m, the slabs of 1 024 frames, the three generic regions of CropsScratch -- and the host
entries' 1 GiB batch loop on that route. Every comparison is byte for byte against oracle.hash_frames on the contiguous numpy
crop; the shapes are the smallest at which the named mechanism is exercised."""
import ctypes as C

import numpy as np
import pytest

import crops_helpers as H
from test_gpu_crops import FILL, check_against_oracle, dct_mode, host_crops, noise
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact
from test_oracle import hard_frames, jarosz_window

pytestmark = pytest.mark.gpu


def transposed(rects):
    return [(left, top, ww, hh) for top, left, hh, ww in rects]


# ---- a. RGB (the luma fused into pass 1, k_luma64_rect<3>) and frames taller than 512 ----

WIDE_CROPS = [(0, 4, 100, 516), (36, 456, 64, 64), (3, 1, 90, 300)]  # the second ends in the last pixel of the last frame


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("tall", [False, True], ids=["100x520", "520x100"])
def test_rgb_and_tall_frames(hvd, gpu, oracle, tall, ch):
    h, w = (520, 100) if tall else (100, 520)
    rects = transposed(WIDE_CROPS) if tall else WIDE_CROPS
    assert all(H.crop_valid(r, h, w) for r in rects) and rects[1][0] + 64 == h and rects[1][1] + 64 == w
    check_against_oracle(hvd, gpu, oracle, noise(30 + 2 * ch + tall, 2, h, w, ch), rects)


# ---- b. both sides above 512: windows 1 to 6 on either axis, left edges at every offset inside a 32-bit word ----

@pytest.mark.parametrize("ch", [1, 3])
def test_both_sides_above_512_around_every_window_change(hvd, gpu, oracle, ch):
    """600 x 700: the sides on both edges of every window change that fits, 128 / 129 ... 640 / 641 on the width and up to
    512 / 513 on the height, the other side alternating between window 5 or 6 and window 1; left % 4 in {1, 2, 3}."""
    h, w = 600, 700
    frames = noise(40 + ch, 2, h, w, ch)
    on_width = [(k, 1 + k % 3, 597 - 2 * k if k % 2 else 100 + k, s)
                for k, s in enumerate((128, 129, 256, 257, 384, 385, 512, 513, 640, 641))]
    on_height = [(k, 1 + k % 3, s, 99 + k if k % 2 else 690 - 3 * k) for k, s in enumerate((128, 129, 256, 257, 384, 385, 512, 513))]
    for rects in (on_width, on_height):
        assert all(H.crop_valid(r, h, w) and r[1] % 4 in (1, 2, 3) for r in rects)
    assert {jarosz_window(r[3]) for r in on_width} == {1, 2, 3, 4, 5, 6} and {jarosz_window(r[2]) for r in on_width} == {1, 5}
    assert {jarosz_window(r[2]) for r in on_height} == {1, 2, 3, 4, 5} and {jarosz_window(r[3]) for r in on_height} == {1, 6}
    for rects in (on_width[:5], on_width[5:], on_height[:4], on_height[4:]):
        check_against_oracle(hvd, gpu, oracle, frames, rects)


# ---- c. K = 7: eight passes over one shared workspace and frame table ----

def test_seven_crops_on_the_generic_route(hvd, gpu, oracle):
    h, w = 530, 96
    rects = [(0, 0, h, w), (3, 1, 500, 90), (466, 32, 64, 64), (17, 0, 64, 96), (3, 1, 500, 90), (2, 29, 513, 64), (9, 2, 385, 70)]
    assert len(rects) == hvd.vpdq.MAX_CROPS and all(H.crop_valid(r, h, w) for r in rects)
    check_against_oracle(hvd, gpu, oracle, noise(50, 3, h, w, 1), rects)


# ---- d. real geometries under the named ladders ----

def _named_ladder(hvd, h, w, crops):
    rects = hvd.vpdq.crop_ladder(h, w, crops)[1]
    assert np.array_equal(rects, H.ladder(h, w, crops)[1])
    return rects


def test_aspect_ladder_on_720p_rgb_hard_content(hvd, gpu, oracle):
    """Noise, stripes, constants and one-pixel impulses in the corners: a crop that misses the impulse is a constant plane of
    quality 0, one that holds it is not."""
    frames, labels = hard_frames(720, 1280, channels=3, seed=2000)
    assert len(labels) == 15
    check_against_oracle(hvd, gpu, oracle, frames, _named_ladder(hvd, 720, 1280, "aspect"), modes=("strict",))


def test_landscape_ladder_on_1080p_rgb(hvd, gpu, oracle):
    rects = _named_ladder(hvd, 1080, 1920, "landscape")
    assert max(jarosz_window(1920), jarosz_window(int(rects[:, 3].max()))) == 15
    check_against_oracle(hvd, gpu, oracle, noise(51, 2, 1080, 1920, 3), rects, modes=("strict",))


def test_portrait_ladder_on_vertical_1080p_gray(hvd, gpu, oracle):
    check_against_oracle(hvd, gpu, oracle, noise(52, 2, 1920, 1080, 1), _named_ladder(hvd, 1920, 1080, "portrait"), modes=("strict",))


# ---- e. the widest windows the route serves ----

def test_windows_31_and_32(hvd, gpu, oracle):
    rects = [(1, 2, 3968, 3969), (127, 64, 3969, 3968), (4032, 4032, 64, 64)]
    assert [jarosz_window(s) for s in (3968, 3969, 4096)] == [31, 32, 32] and all(H.crop_valid(r, 4096, 4096) for r in rects)
    check_against_oracle(hvd, gpu, oracle, noise(53, 1, 4096, 4096, 1), rects, modes=("strict",))


# ---- f. more than one slab: m changes in the last one, and with it every plane base, sk, the CSR and the workspace split ----

def _repeated(seed, n, h, w, ch, distinct=20):
    """n frames, frame f = base[f % distinct]: 20 divides neither 1 024 nor n, so a frame or slot taken from the wrong slab shows."""
    assert 1024 % distinct and n % distinct
    return np.ascontiguousarray(noise(seed, distinct, h, w, ch)[np.arange(n) % distinct])


def test_slab_border_1030_gray(hvd, gpu, oracle):
    """Slabs of 1 024 + 6 frames: a scatter stride or plane base that kept the first slab's 1 024 shows in frames 1024 .. 1029."""
    frames = _repeated(54, 1030, 64, 520, 1)
    check_against_oracle(hvd, gpu, oracle, frames, [(0, 4, 64, 516), (0, 228, 64, 64), (0, 1, 64, 300)], modes=("strict",), distinct=20)


def test_slab_border_1025_rgb_one_frame_tail(hvd, gpu, oracle):
    frames = _repeated(55, 1025, 64, 513, 3)
    check_against_oracle(hvd, gpu, oracle, frames, [(0, 1, 64, 512), (0, 449, 64, 64)], modes=("strict",), distinct=20)


# ---- g. exactly sized buffers: the generic regions of CropsScratch (ws, geom, table) end where the entry says they do ----

def test_exact_scratch_and_outputs_1025_rgb_sentinels(hvd, gpu, oracle):
    """The device entry with n = 1025 RGB 70 x 530 frames and K = 2 in exactly hvd_pdq_crops_scratch_bytes of scratch: the
    64 KiB sentinel tails after the scratch, hash, quality and crop-quality buffers stay intact, the outputs are the oracle's."""
    lib = gpu.load()
    n, h, w, K = 1025, 70, 530, 2
    frames = _repeated(56, n, h, w, 3)
    rects = np.array([(3, 1, 64, 529), (6, 466, 64, 64)], dtype=np.int32)  # both end in the last column, the second in the last pixel
    assert all(H.crop_valid(r, h, w) for r in rects)
    want_h, want_q = H.oracle_crops(oracle, frames[:20], rects)
    idx = np.arange(n) % 20
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_pdq_crops_scratch_bytes(n, h, w, K, C.byref(sb)))
    # one slab of planes, hashes and qualities | the chain's workspace for 1 024 frames | frame table | CSR + 8 rectangles, each
    # region rounded up to 16 bytes: a layout that forgot a region is caught here, before a kernel writes past the buffer
    regions = 1024 * (K + 1) * (4 * 4096 + 32 + 4) + 4 * 1024 * (2 * h * w + 64 * h) + 16 * 1024 + 16 + 16 * 8
    assert regions <= sb.value < regions + 4 * 16, (sb.value, regions)
    d_fr = gpu.DeviceBuffer.from_array(frames)
    sizes = (sb.value, 256 * n, 4 * n, 32 * n)
    bufs = [d_fr] + [_sentinel_buffer(gpu, nbytes) for nbytes in sizes]
    _, d_s, d_h, d_q, d_cq = bufs
    try:
        gpu.check(lib.hvd_dev_pdq_hash_frames_crops(d_fr.ptr, n, h, w, 3, rects.ctypes.data, K, d_s.ptr, d_h.ptr, d_q.ptr, d_cq.ptr))
        gpu.check(lib.hvd_dev_sync())
        h8 = d_h.to_array(np.uint8, 256 * n).reshape(n, 8, 32)
        q, cq = d_q.to_array(np.int32, n), d_cq.to_array(np.int32, 8 * n).reshape(n, 8)
        intact = [_tail_intact(gpu, b, nbytes) for b, nbytes in zip(bufs[1:], sizes)]
    finally:
        for b in bufs:
            b.free()
    assert intact == [True] * 4, ("overrun of (scratch, hashes, quality, crop quality)", intact)
    bad = np.argwhere((h8[:, :K + 1] != want_h[idx]).any(axis=2))
    assert bad.size == 0, ("hashes differ from the oracle at (frame, slot)", bad[:6].tolist())
    assert np.array_equal(cq[:, :K + 1], want_q[idx]) and np.array_equal(q, want_q[idx, 0])
    assert not h8[:, K + 1:].any() and not cq[:, K + 1:].any()


# ---- h. the host entry's 1 GiB batch loop: the second batch is laid out for its own n inside scratch sized for the first ----

def test_host_batch_tail_on_the_generic_route(hvd, gpu, oracle):
    """517 + 1 gray frames of 1080 x 1920 (4 distinct, tiled) under the h9/16 rectangle: frame 517 is a batch of its own."""
    n, h, w = 518, 1080, 1920
    assert (1 << 30) // (h * w) == n - 1
    rects = [(236, 0, 607, 1920)]
    assert np.array_equal(H.ladder(h, w, ("h9/16",))[1], rects)
    base = noise(57, 4, h, w, 1)
    want_h, want_q = H.oracle_crops(oracle, base, rects)
    idx = np.arange(n) % 4
    frames = base[idx]
    with dct_mode(hvd, "strict"):
        h8, q, cq = host_crops(gpu, frames, rects)
    del frames
    bad = np.argwhere((h8[:, :2] != want_h[idx]).any(axis=2))
    assert bad.size == 0, ("hashes differ from the oracle at (frame, slot)", bad[:6].tolist())
    assert np.array_equal(cq[:, :2], want_q[idx]) and np.array_equal(q, want_q[idx, 0])
    assert np.array_equal(h8[517, :2], want_h[517 % 4]) and np.array_equal(cq[517, :2], want_q[517 % 4])
    assert not h8[:, 2:].any() and not cq[:, 2:].any(), "slots above K must be written, as zero"


# ---- i. argument edges at a generic geometry ----

def test_crops_on_and_over_each_border(hvd, gpu, oracle):
    lib = gpu.load()
    h, w = 100, 520
    on = [(36, 0, 64, 200), (0, 320, 90, 200), (0, 3, 100, 64), (2, 0, 64, 520)]  # top = h - hh, left = w - ww, hh = h, ww = w
    over = [(37, 0, 64, 200), (0, 321, 90, 200), (0, 3, 101, 64), (2, 0, 64, 521)]
    frames = noise(58, 2, h, w, 1)
    out, q = np.zeros((2, 8, 32), np.uint8), np.zeros(2, np.int32)
    for k in range(4):
        bad = np.array(on[:k] + [over[k]] + on[k + 1:], dtype=np.int32)
        p = bad.ctypes.data
        assert lib.hvd_dev_pdq_hash_frames_crops(None, 0, h, w, 1, p, 4, None, None, None, None) == gpu.HVD_ERR_ARG, over[k]
        assert lib.hvd_pdq_hash_frames_crops_gray_u8(frames.ctypes.data, 2, h, w, p, 4, out.ctypes.data, q.ctypes.data, None) == gpu.HVD_ERR_ARG
        with pytest.raises(ValueError):
            hvd.vpdq.crop_ladder(h, w, tuple(map(tuple, bad.tolist())))
    assert not out.any() and not q.any()
    check_against_oracle(hvd, gpu, oracle, frames, on)
    sb = C.c_size_t(0)
    for n_, h_, w_, K in ((1, 4097, 520, 1), (1, 100, 4097, 1), (1, 100, 520, 8)):
        assert lib.hvd_pdq_crops_scratch_bytes(n_, h_, w_, K, C.byref(sb)) == gpu.HVD_ERR_ARG
    assert lib.hvd_pdq_crops_scratch_bytes(1, 100, 520, 7, C.byref(sb)) == gpu.HVD_OK and sb.value > 0
