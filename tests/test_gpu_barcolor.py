"""Bar-colour content rectangle on the GPU (run with -m gpu on an MI355X): the colours of the corner pass and
the rectangles of k_content_rect_color against the numpy model (barcolor_helpers), hashes and qualities against the oracle's
over the contiguous crops (autocrop_helpers.oracle_cropped), and the feature end to end. Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import autocrop_helpers as A
import barcolor_helpers as B
from test_gpu_autocrop import shifted_frames
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

WHITE, PILLAR, GREY = (255, 255, 255), (10, 128, 240), (128, 128, 128)
L = 16


# ---- helpers ----

def painted(n, h, w, ch, rect, colour, seed, noise=B.NOISE):
    """n frames of bars (colour +- noise) around uniform random content inside rect = (top, left, hh, ww); gray frames take
    the colour's first channel."""
    rng = np.random.default_rng(seed)
    fr = B.bar_pixels((n, h, w), colour, noise, rng)
    t, l, hh, ww = rect
    fr[:, t:t + hh, l:l + ww] = rng.integers(0, 256, (n, hh, ww, 3), dtype=np.uint8)
    return fr if ch == 3 else np.ascontiguousarray(fr[..., 0])


def join(videos):
    off = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(videos)), off


def pack(colours):
    c = np.asarray(colours, dtype=np.int32)
    return np.ascontiguousarray(sum(c[:, k] << (8 * k) for k in range(c.shape[1])), dtype=np.int32)


def device_chain(gpu, frames, offsets, colours, level=L, bright=1, shift=0):
    """hvd_dev_bar_colors (colours None) -> hvd_dev_content_rects_color -> hvd_dev_pdq_hash_frames_rects, enqueued back to
    back with one synchronisation at the end; every output sits in a sentinel-tailed buffer.
    -> (colours uint8[V,ch], rects int32[V,4], hashes, quality)."""
    lib = gpu.ensure()
    n, h, w = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    V = len(offsets) - 1
    acc, scr = C.c_size_t(0), C.c_size_t(0)
    gpu.check(lib.hvd_bar_colors_scratch_bytes(V, C.byref(acc)))
    gpu.check(lib.hvd_pdq_rects_scratch_bytes(n, h, w, ch, C.byref(scr)))
    assert acc.value == 32 * V
    bufs = []
    try:
        d_fr, fr_ptr = shifted_frames(gpu, frames, shift)
        bufs += [d_fr, gpu.DeviceBuffer.from_array(offsets)]
        for nbytes in (acc.value, 4 * V, 16 * V, scr.value, 32 * n, 4 * n):
            bufs.append(_sentinel_buffer(gpu, nbytes))
        _, d_off, d_acc, d_col, d_rc, d_scr, d_h, d_q = bufs
        if colours is None:
            gpu.check(lib.hvd_dev_bar_colors(fr_ptr, n, h, w, ch, d_off.ptr, V, level, d_acc.ptr, d_col.ptr))
        else:
            packed = pack(colours)
            gpu.check(lib.hvd_memcpy_h2d(d_col.ptr, packed.ctypes.data, packed.nbytes))
        gpu.check(lib.hvd_dev_content_rects_color(fr_ptr, n, h, w, ch, d_off.ptr, V, d_col.ptr, level, bright, d_rc.ptr))
        gpu.check(lib.hvd_dev_pdq_hash_frames_rects(fr_ptr, n, h, w, ch, d_off.ptr, V, d_rc.ptr, d_scr.ptr, d_h.ptr, d_q.ptr))
        gpu.check(lib.hvd_dev_sync())
        packed = d_col.to_array(np.int32, V)
        got = (np.stack([(packed >> (8 * k)) & 0xFF for k in range(ch)], axis=1).astype(np.uint8),
               d_rc.to_array(np.int32, 4 * V).reshape(V, 4), d_h.to_array(np.uint8, 32 * n).reshape(n, 32),
               d_q.to_array(np.int32, n))
        assert (packed >> (8 * ch) == 0).all(), "bits above the channels of the colour record"
        for buf, nbytes, what in ((d_acc, acc.value, "accumulators"), (d_col, 4 * V, "colours"), (d_rc, 16 * V, "rectangles"),
                                  (d_scr, scr.value, "scratch"), (d_h, 32 * n, "hashes"), (d_q, 4 * n, "quality")):
            assert _tail_intact(gpu, buf, nbytes), f"{what} buffer overrun"
    finally:
        for b in bufs:
            b.free()
    return got


def check_case(gpu, hvd, oracle, frames, offsets, colours=None, level=L, bright=1, want_rects=None, want_colours=None,
               shift=0, host=True):
    """Colours and rectangles == the model (device entries, Python entries, host entry); hashes and qualities of the device
    chain and of the host entry == the oracle's over the contiguous crops. colours None: automatic."""
    model_c = B.auto_colors(frames, offsets, level) if colours is None else np.asarray(colours, dtype=np.uint8)
    model_r = B.rule_rects(frames, offsets, model_c, level, bright)
    if want_colours is not None:
        assert model_c.tolist() == np.asarray(want_colours).tolist(), "the case does not build the colours it says"
    if want_rects is not None:
        assert model_r.tolist() == np.asarray(want_rects).tolist(), "the case does not build the rectangles it says"
    wh, wq = A.oracle_cropped(oracle, frames, offsets, model_r)
    dc, dr, dh, dq = device_chain(gpu, frames, offsets, colours, level, bright, shift)
    assert np.array_equal(dc, model_c), (dc.tolist(), model_c.tolist())
    assert np.array_equal(dr, model_r), (dr.tolist(), model_r.tolist())
    assert np.array_equal(dq, wq) and np.array_equal(dh, wh)
    if not host:
        return model_c, model_r
    arg = "auto" if colours is None else model_c
    if colours is None:
        assert np.array_equal(hvd.vpdq.bar_colors(frames, offsets, level), model_c)
    assert np.array_equal(hvd.vpdq.content_rects(frames, offsets, min_bright=bright, bar_color=arg, bar_level=level), model_r)
    h, q, r = hvd.vpdq.hash_frames_autocrop(frames, offsets, min_bright=bright, bar_color=arg, bar_level=level)
    assert np.array_equal(r, model_r)
    assert np.array_equal(q, wq) and np.array_equal(h, wh)
    return model_c, model_r


def three_layouts(n, h, w, ch, seed):
    """White letterbox, a pillar of (10, 128, 240) (three different bytes: the channel order shows), grey windowbox; bars as
    thick as leave 64 (at most 40 a side). -> (frames, offsets, rects, colours are within the noise of the three)."""
    bh, bw = min(40, (h - 64) // 2), min(40, (w - 64) // 2)
    rects = [(bh, 0, h - 2 * bh, w), (0, bw, h, w - 2 * bw), (bh, bw, h - 2 * bh, w - 2 * bw)]
    vids = [painted(n, h, w, ch, rc, c, seed + k) for k, (rc, c) in enumerate(zip(rects, (WHITE, PILLAR, GREY)))]
    return join(vids) + (rects,)


# ---- 1. the geometries: every lane layout of k_content_rect_color, gray and RGB24 ----

GEOMETRIES = [
    (80, 96),     # 6 units, P = 8, WIDE
    (90, 100),    # byte path, width no multiple of 16
    (512, 512),   # P = 32, two rows per wave
    (72, 1040),   # 65 units, P = 128: a row spans waves
]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_three_layouts_at_every_geometry(gpu, hvd, oracle, h, w, ch):
    frames, offsets, rects = three_layouts(2, h, w, ch, seed=h + ch)
    colours, _ = check_case(gpu, hvd, oracle, frames, offsets, want_rects=rects)
    for got, c in zip(colours.astype(int), (WHITE, PILLAR, GREY)):
        assert np.abs(got - c[:ch]).max() <= B.NOISE
    check_case(gpu, hvd, oracle, frames, offsets, colours=colours, want_rects=rects, host=False)


@pytest.mark.parametrize("ch", [1, 3])
def test_unaligned_base_pointer_takes_the_byte_path(gpu, hvd, oracle, ch):
    """512x512 from the device entry with the frames one byte behind an aligned allocation: WIDE is false by alignment."""
    frames, offsets, rects = three_layouts(2, 512, 512, ch, seed=50 + ch)
    check_case(gpu, hvd, oracle, frames, offsets, want_rects=rects, shift=1, host=False)


@pytest.mark.parametrize("ch", [1, 3])
def test_64x64_is_full_by_rule(gpu, hvd, oracle, ch):
    rng = np.random.default_rng(64 + ch)
    fr = B.bar_pixels((4, 64, 64), WHITE, B.NOISE, rng)
    fr[:, 10:50, 10:50] = rng.integers(0, 200, (4, 40, 40, 3), dtype=np.uint8)
    fr = fr if ch == 3 else np.ascontiguousarray(fr[..., 0])
    colours, _ = check_case(gpu, hvd, oracle, fr, np.array([0, 1, 4], np.int64), want_rects=[(0, 0, 64, 64)] * 2)
    assert np.abs(colours.astype(int) - 255).max() <= B.NOISE


# ---- 2. the edges of the rule ----

def letterbox(ch, colour, h=100, w=130, bars=12, n=2, seed=7, noise=0):
    return painted(n, h, w, ch, (bars, 0, h - 2 * bars, w), colour, seed, noise)


@pytest.mark.parametrize("ch", [1, 3])
def test_level_edge_pixels_in_the_outermost_row_and_column(gpu, hvd, oracle, ch):
    c = (100, 120, 140)
    fr = letterbox(ch, c)
    px = (lambda *p: p) if ch == 3 else (lambda *p: p[0])
    full = np.array([0, 2], np.int64)
    fr[0, 0, 129] = px(100 + L, 120 - L, 140 + L)          # |p - c| == L on every channel, in row 0 and column w - 1: bar
    fr[1, 99, 0] = px(100 - L, 120 + L, 140 - L)
    check_case(gpu, hvd, oracle, fr, full, colours=[c[:ch]], want_rects=[(12, 0, 76, 130)])
    fr[1, 99, 0] = px(100 - L - 1, 120, 140) if ch == 1 else (100, 120, 140 - L - 1)   # L + 1 in one channel only: content
    check_case(gpu, hvd, oracle, fr, full, colours=[c[:ch]], want_rects=[(12, 0, 88, 130)])
    fr[0, 0, 129] = px(100 + L + 1, 120, 140) if ch == 1 else (100, 120 + L + 1, 140)
    check_case(gpu, hvd, oracle, fr, full, colours=[c[:ch]], want_rects=[(0, 0, 100, 130)])


@pytest.mark.parametrize("ch", [1, 3])
def test_min_bright_3_ignores_two_stray_pixels_in_a_bar_row(gpu, hvd, oracle, ch):
    fr = letterbox(ch, GREY, noise=B.NOISE)
    fr[0, 3, 40] = fr[0, 3, 90] = 0
    check_case(gpu, hvd, oracle, fr, np.array([0, 2], np.int64), bright=3, want_rects=[(12, 0, 76, 130)])
    check_case(gpu, hvd, oracle, fr, np.array([0, 2], np.int64), bright=2, want_rects=[(3, 0, 85, 130)])
    fr[1, 3, 17] = 0                                       # a third one in the same row of another frame does not add up
    check_case(gpu, hvd, oracle, fr, np.array([0, 2], np.int64), bright=3, want_rects=[(12, 0, 76, 130)])
    fr[0, 3, 17] = 0
    check_case(gpu, hvd, oracle, fr, np.array([0, 2], np.int64), bright=3, want_rects=[(3, 0, 85, 130)])


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("c,bar,content", [(250, 255, 233), (250, 234, 233), (5, 0, 22), (5, 21, 22)])
def test_clamping_near_the_ends_of_the_byte_range(gpu, hvd, oracle, ch, c, bar, content):
    fr = letterbox(ch, (c, c, c))
    off = np.array([0, 2], np.int64)
    fr[1, 2, 0] = bar
    check_case(gpu, hvd, oracle, fr, off, colours=[[c] * ch], want_rects=[(12, 0, 76, 130)])
    check_case(gpu, hvd, oracle, fr, off, want_colours=[[c] * ch], want_rects=[(12, 0, 76, 130)], host=False)
    fr[1, 2, 5] = content
    check_case(gpu, hvd, oracle, fr, off, colours=[[c] * ch], want_rects=[(2, 0, 86, 130)])


# ---- 3. many videos, the fallback to black, explicit colours ----

def test_five_colours_an_empty_video_and_a_one_frame_video(gpu, hvd, oracle):
    cols = (WHITE, (30, 200, 90), GREY, PILLAR, (200, 30, 30))
    rects = [(12, 0, 76, 130), (0, 20, 100, 90), (10, 10, 80, 110), (0, 33, 100, 64), (18, 0, 64, 130)]
    vids = [painted(n, 100, 130, 3, rc, c, 30 + k) for k, (n, rc, c) in enumerate(zip((3, 2, 1, 2, 2), rects, cols))]
    vids.insert(2, np.zeros((0, 100, 130, 3), np.uint8))
    rects.insert(2, (0, 0, 100, 130))
    frames, offsets = join(vids)
    colours, _ = check_case(gpu, hvd, oracle, frames, offsets, want_rects=rects)
    assert colours[2].tolist() == [0, 0, 0]
    # explicit per-video colours equal to the automatic result: the same rectangles and hashes
    check_case(gpu, hvd, oracle, frames, offsets, colours=colours, want_rects=rects)
    # one explicit colour for all videos: only its own video is cropped the same way
    one = hvd.vpdq.content_rects(frames, offsets, bar_color=GREY)
    assert np.array_equal(one, B.rule_rects(frames, offsets, GREY)) and one[3].tolist() == list(rects[3])


@pytest.mark.parametrize("ch", [1, 3])
def test_a_moving_corner_falls_back_to_the_black_rule(gpu, hvd, oracle, ch):
    """The last frame moves one corner by L + 1: automatic gives c = 0 and the rectangle is the black rule's."""
    white = letterbox(ch, (200, 200, 200), n=3, seed=11)
    black = letterbox(ch, (3, 3, 3), n=3, seed=12)
    white[2, 99, 129] = 200 + L + 1
    black[2, 0, 0] = 3 + L + 1
    frames, offsets = join([white, black, white[:2], black[:2]])
    colours, rects = check_case(gpu, hvd, oracle, frames, offsets, want_colours=[[0] * ch, [0] * ch, [200] * ch, [3] * ch],
                                want_rects=[(0, 0, 100, 130), (0, 0, 88, 130), (12, 0, 76, 130), (12, 0, 76, 130)])
    assert np.array_equal(rects[:2], A.rule_rects(frames[:6], offsets[:3], black_level=L))
    assert np.array_equal(hvd.vpdq.content_rects(frames, offsets, black_level=L)[:2], rects[:2])


@pytest.mark.parametrize("ch", [1, 3])
def test_no_bar_colour_is_todays_path_and_colour_zero_is_the_black_rule(gpu, hvd, oracle, ch):
    rng = np.random.default_rng(ch)
    frames = rng.integers(0, 9, (4, 100, 130, 3), dtype=np.uint8)
    frames[:, 15:90, 8:120] = rng.integers(30, 256, (4, 75, 112, 3), dtype=np.uint8)
    frames = frames if ch == 3 else np.ascontiguousarray(frames[..., 0])
    off = np.array([0, 3, 4], np.int64)
    want = A.rule_rects(frames, off, 20, 2)
    assert want.tolist() == [[15, 8, 75, 112]] * 2
    today = hvd.vpdq.content_rects(frames, off, 20, 2)
    assert np.array_equal(today, want)
    assert np.array_equal(hvd.vpdq.content_rects(frames, off, 20, 2, bar_color=None, bar_level=None), today)
    assert np.array_equal(hvd.vpdq.content_rects(frames, off, min_bright=2, bar_color=0, bar_level=20), today)
    t = hvd.vpdq.hash_frames_autocrop(frames, off, 20, 2)
    n = hvd.vpdq.hash_frames_autocrop(frames, off, 20, 2, bar_color=None)
    z = hvd.vpdq.hash_frames_autocrop(frames, off, min_bright=2, bar_color=0, bar_level=20)
    for a, b, c in zip(t, n, z):
        assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- 4. end to end on the 15-video library ----

@pytest.fixture(scope="module")
def library(oracle):
    frames, offsets, rects, groups = B.library_15()
    cropped, _ = A.oracle_cropped(oracle, frames, offsets, rects)
    return frames, offsets, rects, groups, cropped, oracle.match_videos(cropped, offsets, A.FRAME_TOLERANCE)


def test_library_of_15_videos_end_to_end(gpu, hvd, library):
    frames, offsets, rects, groups, cropped, want = library
    from hvd_amd.vpdqpy import Vpdq

    rule = {"bar_color": "auto"}
    h, q, r = hvd.vpdq.hash_frames_autocrop(frames, offsets, bar_color="auto")
    assert np.array_equal(r, rects) and np.array_equal(h, cropped) and q.min() >= 31
    assert np.array_equal(hvd.vpdq.bar_colors(frames, offsets), B.auto_colors(frames, offsets))
    videos = [frames[offsets[v]:offsets[v + 1]] for v in range(15)]
    phashes = hvd.pipeline.hash_videos(videos, autocrop=rule)
    assert [p.bytes for p in phashes] == [h[offsets[v]:offsets[v + 1]].tobytes() for v in range(15)]
    found = hvd.search.find_potential_duplicates(phashes, threshold=50)
    assert found == A.expected_pairs(groups) and len(found) == 30
    for v in (0, 1, 3):
        assert Vpdq.computeHash(videos[v], autocrop=rule).bytes == phashes[v].bytes
    assert Vpdq.computeHash(videos[2], autocrop={"bar_color": B.LIBRARY_COLOURS[0][1], "bar_level": 16}).bytes == phashes[2].bytes
    # the black rule sees bright bars as content: none of the pairs is found
    black = hvd.search.find_potential_duplicates(hvd.pipeline.hash_videos(videos, autocrop=True), threshold=50)
    assert not set(black) & set(found)


def test_pipeline_on_device_with_bar_colour(gpu, hvd, library):
    frames, offsets, rects, groups, cropped, want = library
    d_fr = gpu.DeviceBuffer.from_array(frames)
    try:
        tm = {}
        pairs, recs, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop={"bar_color": "auto"}, timings=tm)
        assert [tuple(p) for p in pairs.tolist()] == A.expected_pairs(groups) and len(pairs) == 30
        assert recs.dtype == want.dtype and np.array_equal(recs, want)
        assert tm["rects_ms"] > 0 and tm["hash_ms"] > 0
        # the host path: the same pairs and records
        h, _, _ = hvd.vpdq.hash_frames_autocrop(frames, offsets, bar_color="auto")
        assert np.array_equal(hvd.search.match_videos(h, offsets, A.FRAME_TOLERANCE), recs)
        explicit = B.auto_colors(frames, offsets)
        p2, r2, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop={"bar_color": explicit, "bar_level": 16})
        assert np.array_equal(p2, pairs) and np.array_equal(r2, recs)
        d_h, d_q, d_r = hvd.pipeline.hash_frames_autocrop_on_device(d_fr.ptr, 120, 512, 512, 3, offsets, bar_color="auto",
                                                                    bar_level=16)
        try:
            assert np.array_equal(d_r.to_array(np.int32, 60).reshape(15, 4), rects)
            assert np.array_equal(d_h.to_array(np.uint8, 32 * 120).reshape(120, 32), cropped)
        finally:
            for b in (d_h, d_q, d_r):
                b.free()
        p0, _, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop=True)
        assert len(p0) == 0
    finally:
        d_fr.free()
