"""VideoHasher(autocrop=...) on the GPU (run with -m gpu on an MI355X): for every case the streamed result --
hashes, qualities, rectangle -- equals vpdq.hash_frames_autocrop on the same frames as one array, byte for byte, and the
rectangle equals the numpy restatement of the rule."""
import ctypes as C

import numpy as np
import pytest

import autocrop_helpers as A
from test_gpu_autocrop import dct_mode, paint

pytestmark = pytest.mark.gpu

FEEDS = ("bytes", "acquire", "acquire_n")


def feed(hs, frames, how):
    ch = 3 if frames.ndim == 4 else 1
    if how == "bytes":
        for f in frames:
            hs.hash_frame(f.tobytes())
    elif how == "acquire":
        for f in frames:
            np.copyto(hs.acquire_frame(ch), f)
            hs.commit_frame()
    else:
        pos = 0
        while pos < len(frames):
            run = hs.acquire_frames(min(7, len(frames) - pos), ch)
            run[:] = frames[pos:pos + len(run)]
            hs.commit_frames()
            pos += len(run)


def raw_finish(gpu, hs):
    """(hashes, quality, rect) of the native finish, unfiltered; ends the hasher."""
    lib = gpu.ensure()
    hs._finished = True
    hs._flush_run()
    n = C.c_int64(0)
    gpu.check(lib.hvd_hasher_pending(hs._handle, C.byref(n)))
    hashes, quality = np.zeros((max(n.value, 1), 32), np.uint8), np.zeros(max(n.value, 1), np.int32)
    got, rect = C.c_int64(0), (C.c_int32 * 4)()
    try:
        gpu.check(lib.hvd_hasher_finish_autocrop(hs._handle, hashes.ctypes.data, quality.ctypes.data, n.value, C.byref(got), rect))
    finally:
        hs.close()
    assert got.value == n.value
    return hashes[:n.value], quality[:n.value], tuple(rect)


def streamed(gpu, hvd, frames, how="bytes", batch_bytes=32 << 20, autocrop=True, h=None, w=None, **kw):
    h, w = (frames.shape[1:3] if h is None else (h, w))
    hs = hvd.vpdq.VideoHasher(1, w, h, 0, batch_bytes=batch_bytes, autocrop=autocrop, **kw)
    if len(frames) == 0:  # the native hasher opens at the first frame: open it by hand
        hs._open(3 if frames.ndim == 4 else 1)
    feed(hs, frames, how)
    return raw_finish(gpu, hs)


def check(gpu, hvd, frames, how="bytes", batch_bytes=32 << 20, level=16, bright=1, want_rect=None):
    """streamed == batch entry == the rule; also through VideoHasher.finish() (quality filter, .rect)."""
    frames = np.ascontiguousarray(frames)
    params = True if (level, bright) == (16, 1) else {"black_level": level, "min_bright": bright}
    h, q, r = streamed(gpu, hvd, frames, how, batch_bytes, params)
    rule = A.rule_rects(frames, None, level, bright)[0] if len(frames) else np.array((0, 0) + frames.shape[1:3])
    if want_rect is not None:
        assert rule.tolist() == list(want_rect), "the case does not build what it says"
    assert list(r) == rule.tolist(), (r, rule)
    if len(frames):
        wh, wq, wr = hvd.vpdq.hash_frames_autocrop(frames, None, level, bright)
        assert wr.tolist() == [rule.tolist()]
    else:
        wh, wq = np.zeros((0, 32), np.uint8), np.zeros(0, np.int32)
    assert np.array_equal(q, wq), np.flatnonzero(q != wq)[:8]
    assert np.array_equal(h, wh), np.flatnonzero((h != wh).any(1))[:8]
    hs = hvd.vpdq.VideoHasher(1, frames.shape[2], frames.shape[1], 0, batch_bytes=batch_bytes, autocrop=params)
    feed(hs, frames, how)
    got = hs.finish()
    assert hs.rect == tuple(rule.tolist())
    assert got.bytes == wh[wq >= 31].tobytes()
    return h, q, r


# ---- the four layouts through the three feeds ----

@pytest.mark.parametrize("how", FEEDS)
def test_the_four_layouts(gpu, hvd, how):
    rng = np.random.default_rng(5)
    for s, (b, ax) in enumerate(A.LAYOUTS):
        fr, rc = A.barred(s, b, ax, rng, nf=12)
        check(gpu, hvd, fr, how, want_rect=rc)


# ---- the case the design exists for: the rectangle grows with a later batch ----

@pytest.mark.parametrize("how", FEEDS)
def test_rectangle_grows_after_many_batches(gpu, hvd, how):
    """40 frames of 256 x 320 RGB, batches of 2 frames (20 batches through 6 slots): dark frames first, then a small box,
    then the box the video ends with."""
    h, w = 256, 320
    fr = np.concatenate([paint(9, h, w, 3, None, 1), paint(13, h, w, 3, (100, 120, 70, 90), 2),
                         paint(11, h, w, 3, (40, 30, 180, 260), 3), paint(7, h, w, 3, (60, 50, 100, 100), 4)])
    check(gpu, hvd, fr, how, batch_bytes=2 * h * w * 3, want_rect=(40, 30, 180, 260))


def test_rectangle_grows_in_the_last_frame(gpu, hvd):
    h, w = 200, 300
    fr = np.concatenate([paint(30, h, w, 1, (50, 60, 80, 100), 5), paint(1, h, w, 1, (3, 5, 190, 290), 6)])
    check(gpu, hvd, fr, batch_bytes=4 * h * w, want_rect=(3, 5, 190, 290))


# ---- the rule's corners ----

def test_no_bars_all_dark_narrow_content_and_a_dark_frame_in_the_middle(gpu, hvd):
    h, w = 240, 320
    check(gpu, hvd, paint(6, h, w, 3, (0, 0, h, w), 10), want_rect=(0, 0, h, w))
    check(gpu, hvd, paint(6, h, w, 3, None, 11), want_rect=(0, 0, h, w))
    check(gpu, hvd, paint(6, h, w, 3, (10, 16, 200, 40), 12), want_rect=(10, 0, 200, w))      # 40 columns: full width
    fr = paint(7, h, w, 3, (20, 30, 200, 250), 13)
    fr[3] = paint(1, h, w, 3, None, 14)[0]
    check(gpu, hvd, fr, batch_bytes=h * w * 3, want_rect=(20, 30, 200, 250))
    check(gpu, hvd, paint(5, h, w, 1, (20, 30, 200, 250), 15, lo=60), level=50, bright=3, want_rect=(20, 30, 200, 250))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_very_short_videos(gpu, hvd, n):
    fr = paint(n, 128, 160, 3, (9, 16, 100, 112), 20)
    _, _, r = check(gpu, hvd, fr)
    assert r == ((9, 16, 100, 112) if n else (0, 0, 128, 160))


def test_a_64x64_video_and_a_geometry_above_512(gpu, hvd):
    check(gpu, hvd, hvd.synth.frames_gray(300, seed=21), want_rect=(0, 0, 64, 64))
    check(gpu, hvd, np.random.default_rng(22).integers(0, 256, (40, 64, 64, 3), dtype=np.uint8), "acquire_n")
    check(gpu, hvd, paint(5, 720, 1280, 1, (90, 0, 540, 1280), 23), want_rect=(90, 0, 540, 1280))


def test_both_dct_modes(gpu, hvd):
    fr, rc = A.barred(3, 64, "h", np.random.default_rng(30), nf=10)
    with dct_mode(hvd, "fma"):
        hf, _, _ = check(gpu, hvd, fr, want_rect=rc)
    hs, _, _ = check(gpu, hvd, fr, want_rect=rc)
    assert hf.shape == hs.shape


# ---- parked slots, interleaved hashers ----

def test_second_video_through_a_new_hasher_of_the_same_geometry(gpu, hvd):
    h, w = 256, 256
    big = paint(20, h, w, 3, (2, 3, 250, 250), 40)
    small = paint(9, h, w, 3, (90, 80, 70, 100), 41)
    for fr, rc in ((big, (2, 3, 250, 250)), (small, (90, 80, 70, 100)), (paint(3, h, w, 3, None, 42), (0, 0, h, w)), (small[:0], None)):
        check(gpu, hvd, fr, batch_bytes=3 * h * w * 3, want_rect=rc)
    # a video that is abandoned (no finish) leaves nothing behind either
    hs = hvd.vpdq.VideoHasher(1, w, h, 0, batch_bytes=3 * h * w * 3, autocrop=True)
    feed(hs, big, "bytes")
    hs.close()
    check(gpu, hvd, small, batch_bytes=3 * h * w * 3, want_rect=(90, 80, 70, 100))


def test_plain_and_autocrop_hashers_interleaved(gpu, hvd):
    fr, rc = A.barred(2, 96, "h", np.random.default_rng(50), nf=16)
    plain = hvd.vpdq.VideoHasher(1, 512, 512, 0, batch_bytes=3 * 512 * 512 * 3)
    crop = hvd.vpdq.VideoHasher(1, 512, 512, 0, batch_bytes=3 * 512 * 512 * 3, autocrop=True)
    for f in fr:
        plain.hash_frame(f.tobytes())
        crop.hash_frame(f.tobytes())
    ph, pq = hvd.vpdq.hash_frames(fr)
    ch, cq, cr = hvd.vpdq.hash_frames_autocrop(fr)
    assert plain.finish().bytes == ph[pq >= 31].tobytes()
    assert crop.finish().bytes == ch[cq >= 31].tobytes() and crop.rect == tuple(cr[0].tolist()) == rc
    assert not np.array_equal(ph, ch)


# ---- the cap, wrong-kind calls ----

def test_max_retained_bytes_and_wrong_kind_finish(gpu, hvd):
    lib = gpu.ensure()
    h, w = 128, 160
    fr = paint(5, h, w, 3, (9, 16, 100, 112), 60)
    hs = hvd.vpdq.VideoHasher(1, w, h, 0, autocrop=True, max_retained_bytes=3 * h * w * 3 + 5)
    for f in fr[:3]:
        hs.hash_frame(f.tobytes())
    with pytest.raises(gpu.HvdError) as e:
        hs.hash_frame(fr[3].tobytes())
    assert e.value.code == gpu.HVD_ERR_OVERFLOW
    with pytest.raises(gpu.HvdError) as e:
        hs.acquire_frame(3)
    assert e.value.code == gpu.HVD_ERR_OVERFLOW
    out, q, n = np.zeros((8, 8, 32), np.uint8), np.zeros(8, np.int32), C.c_int64(0)
    assert lib.hvd_hasher_finish(hs._handle, out.ctypes.data, q.ctypes.data, 8, C.byref(n)) == gpu.HVD_ERR_STATE
    assert lib.hvd_hasher_finish_dihedral(hs._handle, out.ctypes.data, q.ctypes.data, 8, C.byref(n)) == gpu.HVD_ERR_STATE
    got_h, got_q, got_r = raw_finish(gpu, hs)
    wh, wq, wr = hvd.vpdq.hash_frames_autocrop(fr[:3])
    assert np.array_equal(got_h, wh) and np.array_equal(got_q, wq) and got_r == tuple(wr[0].tolist()) == (9, 16, 100, 112)
    # a run is cut to what the cap leaves
    hs = hvd.vpdq.VideoHasher(1, w, h, 0, autocrop=True, max_retained_bytes=3 * h * w * 3)
    run = hs.acquire_frames(5, 3)
    assert len(run) == 3
    run[:] = fr[:3]
    hs.commit_frames()
    got_h, _, _ = raw_finish(gpu, hs)
    assert np.array_equal(got_h, wh)
    # the other kinds refuse the autocrop finish; bad parameters are refused at create
    rect = (C.c_int32 * 4)()
    for kw in ({}, {"transforms": "mirror"}):
        other = hvd.vpdq.VideoHasher(1, w, h, 0, **kw)
        other.hash_frame(fr[0].tobytes())
        assert lib.hvd_hasher_finish_autocrop(other._handle, out.ctypes.data, q.ctypes.data, 8, C.byref(n), rect) == gpu.HVD_ERR_STATE
        other.close()
    hd = C.c_void_p()
    for level, bright in ((-1, 1), (255, 1), (16, 0)):
        assert lib.hvd_hasher_create_autocrop(w, h, 3, 4, level, bright, 0, C.byref(hd)) == gpu.HVD_ERR_ARG


# ---- end to end: the premise ----

def test_streamed_barred_copy_is_found_only_with_autocrop(gpu, hvd):
    original = A.content(512, 512, 1, nf=8)
    copy, rc = A.barred(1, 64, "h", np.random.default_rng(70))

    def stream(fr, **kw):
        hs = hvd.vpdq.VideoHasher(1, 512, 512, 0, **kw)
        for f in fr:
            hs.hash_frame(f.tobytes())
        return hs.finish(), hs.rect

    (a, ra), (b, rb) = stream(original, autocrop=True), stream(copy, autocrop=True)
    assert ra == (0, 0, 512, 512) and rb == rc
    ha = np.frombuffer(a.bytes, np.uint8).reshape(-1, 32)
    hb = np.frombuffer(b.bytes, np.uint8).reshape(-1, 32)
    assert len(ha) == len(hb) == 8
    d = A.hamming(ha, hb)
    print("streamed with autocrop, frame by frame:", d.tolist())
    assert d.max() <= A.FRAME_TOLERANCE
    assert hvd.search.find_potential_duplicates([a, b], threshold=50) == [(0, 1)]
    (a0, _), (b0, _) = stream(original), stream(copy)
    h0a = np.frombuffer(a0.bytes, np.uint8).reshape(-1, 32)
    h0b = np.frombuffer(b0.bytes, np.uint8).reshape(-1, 32)
    print("streamed without:", A.hamming(h0a, h0b).tolist())
    assert A.hamming(h0a, h0b).min() > A.FRAME_TOLERANCE
    assert hvd.search.find_potential_duplicates([a0, b0], threshold=50) == []
