"""The fused rectangle down-sampler k_down_rect (run with -m gpu on an MI355X): planes, hashes and qualities of
hvd_dev_pdq_hash_frames_rects with the debug key pdq_fused_rect at 1 against oracle.planes64 / the oracle's hashes over the
contiguous crops, every float bit for bit, and against the same call with the key at 0 (the four generic passes). The
scratch layout contract (the 64x64 planes lead the scratch) is what makes the planes readable."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import autocrop_helpers as A
from test_gpu_autocrop import dct_mode, device_rect_hash, join

pytestmark = pytest.mark.gpu

SIDES = (64, 65, 128, 129, 256, 257, 384, 385, 512)  # both ends of the range of every window 1..4


@contextlib.contextmanager
def fused(gpu, on):
    lib = gpu.ensure()
    gpu.check(lib.hvd_debug_set(b"pdq_fused_rect", int(on)))
    try:
        yield
    finally:
        gpu.check(lib.hvd_debug_set(b"pdq_fused_rect", 1))


def noise(n, h, w, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) if ch == 1 else (n, h, w, 3), dtype=np.uint8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(gpu, hvd, oracle, frames, offsets, rects, effective=None, shift=0, modes=("strict", "fma")):
    """rects go to the device as they are; `effective` is what the device must make of them (records outside the frame
    become the full frame)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rects = np.asarray(rects, dtype=np.int32).reshape(-1, 4)
    eff = rects if effective is None else np.asarray(effective, dtype=np.int32).reshape(-1, 4)
    wh, wq, wp = A.oracle_cropped(oracle, frames, offsets, eff, planes=True)
    for mode in modes:
        with dct_mode(hvd, mode):
            if mode == "fma":
                wh, wq = A.oracle_cropped(oracle, frames, offsets, eff, fma=True)
            with fused(gpu, 1):
                p1, h1, q1 = device_rect_hash(gpu, frames, offsets, rects, shift=shift)
            with fused(gpu, 0):
                p0, h0, q0 = device_rect_hash(gpu, frames, offsets, rects, shift=shift)
            bad = np.flatnonzero((bits(p1) != bits(wp)).any(axis=(1, 2)))
            if bad.size:
                f = int(bad[0])
                v = int(np.searchsorted(offsets, f, side="right") - 1)
                ij = np.argwhere(bits(p1[f]) != bits(wp[f]))
                print(f"{mode}: {bad.size} planes differ; first frame {f}, rect {eff[v].tolist()}, {len(ij)} cells, "
                      f"first {ij[:6].tolist()}, got {p1[f][tuple(ij[0])]!r} want {wp[f][tuple(ij[0])]!r}")
            assert bad.size == 0, (mode, f"{bad.size} planes differ from the oracle's, first frame {bad[0]}")
            assert np.array_equal(bits(p1), bits(p0)), (mode, "fused and generic planes differ")
            assert np.array_equal(h1, wh) and np.array_equal(q1, wq), mode
            assert np.array_equal(h1, h0) and np.array_equal(q1, q0), mode


def one_video_per_rect(n_each, h, w, ch, rects, seed):
    vids = [noise(n_each, h, w, ch, seed + i) for i in range(len(rects))]
    return join(vids)


# ---- every pair of windows, both ends of each window's range, odd origins ----

@pytest.mark.parametrize("ch", [1, 3])
def test_every_window_pair_at_odd_origins(gpu, hvd, oracle, ch):
    h = w = 512
    rects = []
    for i, hh in enumerate(SIDES):
        for j, ww in enumerate(SIDES):
            top = min(h - hh, 1 + 2 * ((3 * i + j) % 40))   # odd wherever the rectangle leaves room
            left = min(w - ww, 1 + 2 * ((5 * j + i) % 37))
            rects.append((top, left, hh, ww))
    assert len(rects) == 81 and sum(r[0] % 2 == 1 and r[1] % 2 == 1 for r in rects) >= 60
    frames, off = one_video_per_rect(1, h, w, ch, rects, 100)
    check(gpu, hvd, oracle, frames, off, rects, modes=("strict", "fma") if ch == 3 else ("strict",))


@pytest.mark.parametrize("ch", [1, 3])
def test_rectangles_touching_each_frame_edge(gpu, hvd, oracle, ch):
    h, w = 500, 508
    rects = [(0, 37, 300, 401), (200, 37, 300, 401), (37, 0, 301, 400), (37, 108, 301, 400), (0, 0, 257, 129),
             (243, 379, 257, 129), (0, 443, 500, 65), (435, 0, 65, 508), (436, 444, 64, 64), (0, 0, 64, 64)]
    frames, off = one_video_per_rect(2, h, w, ch, rects, 200)
    check(gpu, hvd, oracle, frames, off, rects, modes=("strict",))


@pytest.mark.parametrize("h,w", [(512, 512), (511, 512), (512, 511), (512, 480), (360, 480), (480, 360), (65, 512), (512, 65),
                                 (64, 65), (81, 85)])
@pytest.mark.parametrize("ch", [1, 3])
def test_full_rectangles(gpu, hvd, oracle, h, w, ch):
    """The rectangle is the whole frame, among them widths that are no multiple of 16 (or of 4)."""
    frames = noise(3, h, w, ch, 300 + h + w)
    check(gpu, hvd, oracle, frames, [0, 3], [(0, 0, h, w)], modes=("strict",))
    if (h, w) == (512, 512):  # ... where the plain fused kernels give the same hashes
        with fused(gpu, 1):
            _, hh, qq = device_rect_hash(gpu, frames, np.array([0, 3], np.int64), np.array([(0, 0, h, w)], np.int32))
        ph, pq = hvd.vpdq.hash_frames(frames)
        assert np.array_equal(hh, ph) and np.array_equal(qq, pq)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("h,w", [(300, 333), (257, 391)])
def test_widths_that_are_no_multiple_of_16(gpu, hvd, oracle, h, w, ch):
    rects = [(3, 5, 250, 300), (0, 1, 129, 257), (1, 2, 64, 70), (0, 0, h, w), (7, 0, 200, w), (0, 9, h, 128)]
    frames, off = one_video_per_rect(2, h, w, ch, rects, 400)
    check(gpu, hvd, oracle, frames, off, rects, modes=("strict",))


@pytest.mark.parametrize("ch", [1, 3])
def test_frames_at_an_odd_device_address(gpu, hvd, oracle, ch):
    rects = [(9, 16, 100, 112), (0, 0, 128, 160), (1, 3, 127, 157), (63, 95, 65, 65)]
    frames, off = one_video_per_rect(2, 128, 160, ch, rects, 500)
    for shift in (1, 2, 3, 5, 8):
        check(gpu, hvd, oracle, frames, off, rects, shift=shift, modes=("strict",))


def test_many_rectangles_in_one_launch_across_the_slab_border(gpu, hvd, oracle):
    """1 300 frames of 160 x 192 RGB in 325 videos with 12 different rectangles: more frames than the fused kernel's grid has
    workgroups (256), and more than one 1024-frame slab of the generic path."""
    h, w = 160, 192
    kinds = [(0, 0, h, w), (1, 1, 129, 129), (31, 63, 128, 128), (0, 0, 64, 64), (5, 7, 64, 65), (3, 0, 65, 64), (96, 128, 64, 64),
             (11, 13, 130, 170), (0, 63, 160, 129), (29, 0, 131, 192), (2, 2, 156, 188), (17, 33, 100, 150)]
    V = 325
    frames = noise(4 * V, h, w, 3, 600)
    off = np.arange(0, 4 * V + 1, 4, dtype=np.int64)
    rects = [kinds[(7 * v) % len(kinds)] for v in range(V)]
    assert len(frames) > 1024 + 256
    check(gpu, hvd, oracle, frames, off, rects, modes=("strict",))


def test_records_outside_the_frame_are_the_full_frame(gpu, hvd, oracle):
    h, w = 200, 300
    full = (0, 0, h, w)
    bad = [(-1, 0, 100, 100), (0, -3, 100, 100), (101, 0, 100, 100), (0, 201, 100, 100), (0, 0, 63, 100), (0, 0, 100, 63),
           (0, 0, 201, 300), (0, 0, 200, 301), (2 ** 31 - 1, 0, 64, 64), (0, 0, -5, 64), (10, 20, 100, 120)]
    frames, off = one_video_per_rect(1, h, w, 3, bad, 700)
    check(gpu, hvd, oracle, frames, off, bad, effective=[full] * 10 + [bad[-1]], modes=("strict",))


def test_no_frames(gpu):
    lib = gpu.ensure()
    d = [gpu.DeviceBuffer(64) for _ in range(5)]
    try:
        with fused(gpu, 1):
            gpu.check(lib.hvd_dev_pdq_hash_frames_rects(d[0].ptr, 0, 512, 512, 3, d[1].ptr, 1, d[2].ptr, d[3].ptr, d[4].ptr, d[4].ptr))
            gpu.check(lib.hvd_dev_sync())
    finally:
        for b in d:
            b.free()


@pytest.mark.parametrize("h,w", [(512, 513), (513, 512)])
def test_frames_above_512_keep_the_generic_path(gpu, hvd, oracle, h, w):
    rects = [(1, 1, 400, 500), (0, 0, h, w), (100, 200, 129, 257)]
    frames, off = one_video_per_rect(2, h, w, 3, rects, 800)
    check(gpu, hvd, oracle, frames, off, rects, modes=("strict",))


def test_scratch_need_is_unchanged(gpu):
    """hvd_pdq_rects_scratch_bytes does not depend on the key: the fused path uses the head of the same scratch."""
    lib = gpu.ensure()
    got = []
    for on in (1, 0):
        with fused(gpu, on):
            sb = C.c_size_t(0)
            gpu.check(lib.hvd_pdq_rects_scratch_bytes(300, 512, 512, 3, C.byref(sb)))
            got.append(sb.value)
    assert got[0] == got[1] > 300 * 4096 * 4
