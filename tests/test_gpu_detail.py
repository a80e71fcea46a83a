"""Detail content rectangle on the GPU (run with -m gpu on an MI355X): the rectangles of k_content_rect_detail
against the numpy model (detail_helpers) at the rule's thresholds and at every boundary of the kernel's decomposition, hashes
and qualities against the oracle's over the contiguous crops, and the feature end to end. Every comparison is equality.

The kernel cases give each video one frame, so one launch checks many frames. A case frame is flat (value 100) around a
0 / 255 checkerboard BLOCK at rows 1..64 x columns 1..64 -- detail at any level, a box of 64 x 64 that the fallback keeps --
and carries one PROBE in the flat margin: a single neighbour pair that differs, which moves one side of the rectangle iff the
kernel sees exactly that pair."""
import ctypes as C

import numpy as np
import pytest

import autocrop_helpers as A
import detail_helpers as D
from test_gpu_autocrop import dct_mode, shifted_frames
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

FLAT = 100
BLOCK = (1, 1, 64, 64)


# ---- helpers ----

def device_rects(gpu, frames, offsets, level=8, count=8, shift=0, n=None):
    """hvd_dev_content_rects_detail into a sentinel-tailed int32[V][4] buffer. n: frames to launch (default: all)."""
    lib = gpu.ensure()
    h, w = frames.shape[1:3]
    n = frames.shape[0] if n is None else n
    V = len(offsets) - 1
    d_fr, fr_ptr = shifted_frames(gpu, frames, shift)
    bufs = [d_fr, gpu.DeviceBuffer.from_array(np.ascontiguousarray(offsets, dtype=np.int64)), _sentinel_buffer(gpu, 16 * V)]
    try:
        gpu.check(lib.hvd_dev_content_rects_detail(fr_ptr, n, h, w, 3 if frames.ndim == 4 else 1, bufs[1].ptr, V, level, count,
                                                   bufs[2].ptr))
        gpu.check(lib.hvd_dev_sync())
        got = bufs[2].to_array(np.int32, 4 * V).reshape(V, 4)
        assert _tail_intact(gpu, bufs[2], 16 * V), "rectangle buffer overrun"
    finally:
        for b in bufs:
            b.free()
    return got


def one_each(frames):
    return np.arange(len(frames) + 1, dtype=np.int64)


def check(gpu, frames, offsets=None, level=8, count=8, want=None, shift=0):
    """device rectangles == the model; want: what the case says it builds."""
    frames = np.ascontiguousarray(frames)
    offsets = np.array([0, len(frames)], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    model = D.rule_rects(frames, offsets, level, count)
    if want is not None:
        assert model.tolist() == [list(r) for r in want], "the case does not build what it says"
    got = device_rects(gpu, frames, offsets, level, count, shift)
    assert np.array_equal(got, model), [(v, g, m) for v, (g, m) in enumerate(zip(got.tolist(), model.tolist())) if g != m][:8]
    return model


def base(h, w, ch, block=BLOCK, flat=FLAT):
    """One flat frame with the checkerboard block. uint8[h,w] / uint8[h,w,3]."""
    fr = np.full((h, w, ch), flat, np.uint8)
    t, l, hh, ww = block
    yy, xx = np.mgrid[t:t + hh, l:l + ww]
    fr[t:t + hh, l:l + ww] = (((yy + xx) & 1) * 255)[..., None]
    return fr if ch == 3 else fr[..., 0]


def _steps(line, cuts, d, split):
    """A flat line (1-D view, all channels or one) cut after the positions `cuts` into segments that alternate between
    flat - a and flat + d - a, a = d / 2 towards zero (split) or 0: neighbours differ by |d| across every cut and nowhere
    else, and no value is further than max(|a|, |d - a|) from the flat lines beside it."""
    a = int(d / 2) if split else 0
    edges = [0] + [c + 1 for c in cuts] + [line.shape[0]]
    for i in range(len(edges) - 1):
        seg = line[edges[i]:edges[i + 1]]
        seg[...] = seg.astype(np.int64) + (-a if i % 2 == 0 else d - a)


def h_probe(fr, y, x, d=9, k=None, split=True):
    """Row y differs by d between columns x and x + 1 (x: an int or several) and nowhere else along the row; with split, the
    row stays within |d| / 2 (rounded up) of the rows beside it, so for |d| <= 2 L no vertical pair is above L."""
    fr = fr.copy()
    _steps(fr[y] if fr.ndim == 2 or k is None else fr[y, :, k], [x] if np.isscalar(x) else list(x), d, split)
    return fr


def v_probe(fr, y, x, d=9, k=None, split=True):
    """Column x differs by d between rows y and y + 1 (y: an int or several) and nowhere else along the column."""
    fr = fr.copy()
    _steps(fr[:, x] if fr.ndim == 2 or k is None else fr[:, x, k], [y] if np.isscalar(y) else list(y), d, split)
    return fr


def decomposition(h, w):
    """(units, P, R, B) of k_content_rect_detail: 16-pixel units, P lanes per row segment, R lane-rows, B rows per band."""
    units = (w + 15) // 16
    P = 1
    while P < units:
        P <<= 1
    R = 256 // P
    return units, P, R, (h + R - 1) // R


# ---- 1. thresholds ----

@pytest.mark.parametrize("ch,h,w", [(3, 100, 130), (1, 100, 130), (3, 96, 128)])
def test_level_edges_channels_and_signs(gpu, ch, h, w):
    """The probe sits in row 80 (horizontal) or column 90 (vertical), outside the block: seen -> the box grows to it."""
    L = 8
    b = base(h, w, ch)
    seen_h, seen_v, unseen = (1, 1, 80, 64), (1, 1, 64, 90), BLOCK
    cases = [(h_probe(b, 80, 40, L), unseen), (h_probe(b, 80, 40, L + 1), seen_h), (h_probe(b, 80, 40, -L), unseen),
             (h_probe(b, 80, 40, -L - 1), seen_h), (v_probe(b, 30, 90, L), unseen), (v_probe(b, 30, 90, L + 1), seen_v),
             (v_probe(b, 30, 90, -L - 1), seen_v), (v_probe(b, 30, 90, -L), unseen)]
    for k in range(ch if ch == 3 else 0):  # one channel only, each of the three
        cases += [(h_probe(b, 80, 40, L + 1, k), seen_h), (h_probe(b, 80, 40, L, k), unseen),
                  (v_probe(b, 30, 90, -L - 1, k), seen_v), (v_probe(b, 30, 90, L, k), unseen)]
    frames = np.stack([c[0] for c in cases])
    check(gpu, frames, one_each(frames), L, 1, want=[c[1] for c in cases])


@pytest.mark.parametrize("ch", [1, 3])
def test_level_0_and_254_and_0_against_255(gpu, ch):
    """At L = 0 a step of 1 is detail along both axes, so only the side the probe is about is stated here."""
    h, w = 100, 130
    b = base(h, w, ch)
    one = np.stack([h_probe(b, 80, 40, 1), v_probe(b, 30, 90, -1), b])
    m = check(gpu, one, one_each(one), 0, 1)
    assert m[0, [0, 2]].tolist() == [1, 80] and m[1, [1, 3]].tolist() == [1, 90] and m[2].tolist() == list(BLOCK)
    dark = base(h, w, ch, flat=0)
    hi = np.stack([h_probe(dark, 80, 40, 255, split=False), h_probe(dark, 80, 40, 254, split=False),
                   v_probe(dark, 30, 90, 255, split=False), v_probe(dark, 30, 90, 254, split=False)])
    # at 254 only 0 | 255 differs: the block's own pairs and the probes of 255 (which the other axis sees as well)
    m = check(gpu, hi, one_each(hi), 254, 1)
    assert m[0, [0, 2]].tolist() == [1, 80] and m[2, [1, 3]].tolist() == [1, 90] and m[[1, 3]].tolist() == [list(BLOCK)] * 2
    if ch == 3:
        k1 = np.stack([h_probe(dark, 80, 40, 255, 1, split=False), v_probe(dark, 30, 90, 255, 2, split=False)])
        m = check(gpu, k1, one_each(k1), 254, 1)
        assert m[0, [0, 2]].tolist() == [1, 80] and m[1, [1, 3]].tolist() == [1, 90]


@pytest.mark.parametrize("ch", [1, 3])
def test_count_below_and_at_min_detail(gpu, ch):
    """m = 3: two pairs in a row (column) are not content, three are; pairs of other frames of the video do not add up."""
    h, w = 100, 130
    b = base(h, w, ch)
    two_h, three_h = h_probe(b, 80, (40, 70)), h_probe(b, 80, (40, 70, 100))
    two_v, three_v = v_probe(b, (20, 50), 90), v_probe(b, (20, 50, 75), 90)
    frames = np.stack([two_h, three_h, two_v, three_v])
    check(gpu, frames, one_each(frames), 8, 3, want=[BLOCK, (1, 1, 80, 64), BLOCK, (1, 1, 64, 90)])
    check(gpu, frames, one_each(frames), 8, 2, want=[(1, 1, 80, 64), (1, 1, 80, 64), (1, 1, 64, 90), (1, 1, 64, 90)])
    split = np.stack([two_h, h_probe(b, 80, 100), two_v, v_probe(b, 75, 90)])
    check(gpu, split, [0, 2, 4], 8, 3, want=[BLOCK, BLOCK])


# ---- 2. edges: the last pairs, the fallback at 63 | 64 ----

@pytest.mark.parametrize("ch,h,w", [(3, 100, 130), (1, 96, 128), (3, 96, 128)])
def test_last_column_pair_and_last_row_pair(gpu, ch, h, w):
    b = base(h, w, ch)
    frames = np.stack([h_probe(b, 80, w - 2), v_probe(b, h - 2, 90), h_probe(b, h - 1, w - 2), v_probe(b, h - 2, w - 1),
                       h_probe(b, 0, 0), v_probe(b, 0, 0)])
    check(gpu, frames, one_each(frames), 8, 1,
          want=[(1, 1, 80, 64), (1, 1, 64, 90), (1, 1, h - 1, 64), (1, 1, 64, w - 1), (0, 1, 65, 64), (1, 0, 64, 65)])


@pytest.mark.parametrize("ch", [1, 3])
def test_box_of_63_keeps_the_full_extent_and_64_is_kept(gpu, ch):
    h, w = 100, 130
    frames = np.stack([base(h, w, ch, (5, 7, 64, 64)), base(h, w, ch, (5, 7, 63, 64)), base(h, w, ch, (5, 7, 64, 63)),
                       base(h, w, ch, (5, 7, 63, 63))])
    check(gpu, frames, one_each(frames), 8, 8, want=[(5, 7, 64, 64), (0, 7, 100, 64), (5, 0, 64, 130), (0, 0, 100, 130)])


# ---- 3. geometries: a probe at every boundary of the decomposition ----

GEOMETRIES = [
    (80, 96, 1, 0),      # 6 units, P = 8, 32 lane-rows of 3 rows: h is no multiple of the band count
    (80, 96, 3, 0),
    (72, 200, 3, 0),     # byte form: the width is no multiple of 16, the last unit holds 8 pixels
    (72, 200, 1, 0),
    (512, 512, 3, 1),    # a WIDE-eligible shape one byte behind an aligned base: byte form by alignment
    (130, 1040, 3, 0),   # 65 units, P = 128: a row segment spans two waves, x = 1023 | 1024 is a wave edge
    (130, 1040, 1, 0),
    (65, 2064, 3, 0),    # 129 units, P = 256: one lane-row, one band of 65 rows, four waves per row
    (512, 512, 3, 0),    # P = 32: two row segments per wave, 8 bands of 64 rows
    (100, 512, 1, 0),    # 8 bands of 13 rows: the last band is short
]


def boundary_probes(h, w, ch):
    """[(frame, which side must move)]: horizontal pairs in margin rows (0, and >= 65 where the frame has them) at x = 0, 7,
    every unit boundary that is a segment or wave edge (16 * 64 * k - 1), the first and the last unit boundary, w - 2; in the
    first and last row of bands outside the block. Vertical pairs in the margin columns 0 and w - 1 at y = 0, every band
    boundary (first, second and last of them), h - 2. Plus the row end: pixel w - 1 of a row against pixel 0 of the next row
    is no pair."""
    units, P, R, B = decomposition(h, w)
    b = base(h, w, ch)
    out = []
    xs = {0, 7, 15, 16 * (units - 1) - 1, w - 2} | {x for x in range(1023, w - 1, 1024)} | {16 * (P // 2) - 1}
    rows = {0} | {y for r in range(R) for y in (r * B, r * B + B - 1) if 65 <= y < h}
    rows = sorted(rows)[:1] + sorted(rows)[1:4] + sorted(rows)[-2:]
    for y in sorted(set(rows)):
        for x in sorted(x for x in xs if 0 <= x <= w - 2):
            out.append((h_probe(b, y, x), "row"))
    edges = [r * B - 1 for r in range(1, R) if r * B < h]
    ys = {0, h - 2} | set(edges[:2]) | set(edges[-1:])
    for y in sorted(ys):
        for x in (0, w - 1):
            out.append((v_probe(b, y, x), "column"))
    if h > 67:  # rows 66 and 67 differ in every column, pixel (66, w - 1) | (67, 0) included: columns are content, no row is
        fr = b.copy()
        fr[67] = FLAT + 9
        out.append((fr, "columns"))
    return out


@pytest.mark.parametrize("h,w,ch,shift", GEOMETRIES)
def test_a_probe_at_every_boundary_of_the_decomposition(gpu, h, w, ch, shift):
    probes = boundary_probes(h, w, ch)
    frames = np.stack([p[0] for p in probes])
    model = check(gpu, frames, one_each(frames), 8, 1, shift=shift)
    for (_, side), (t, l, hh, ww) in zip(probes, model.tolist()):  # every probe is visible in the model's rectangle
        if side == "row":
            assert (l, ww) == (1, 64) and (t, hh) != (1, 64)
        elif side == "column":
            assert (t, hh) == (1, 64) and (l, ww) != (1, 64)
        else:
            assert (t, l, hh, ww) == (1, 0, 64, w)


@pytest.mark.parametrize("ch", [1, 3])
def test_64x64_is_full_by_rule(gpu, ch):
    rng = np.random.default_rng(ch)
    fr = rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)
    fr[:, :10] = 50
    fr = fr if ch == 3 else np.ascontiguousarray(fr[..., 0])
    check(gpu, fr, [0, 1, 3], want=[(0, 0, 64, 64)] * 2)


@pytest.mark.parametrize("h,w,ch", [(80, 96, 3), (72, 200, 1), (130, 1040, 3), (512, 512, 3), (65, 2064, 1)])
def test_random_texture_inside_flat_bars_at_the_defaults(gpu, h, w, ch):
    """Uniform random content inside a rectangle, bars of a slow ramp with +-2 noise: L = 8, m = 8."""
    rng = np.random.default_rng(h + w + ch)
    ramp = (30 + (np.arange(w) * 100) // w)[None, None, :, None]
    fr = np.clip(ramp + rng.integers(-2, 3, (3, h, w, 3)), 0, 255).astype(np.uint8)
    t, l = (h - 64) // 3, (w - 64) // 3
    hh, ww = h - t - (h - 64 - t) // 2, w - l - (w - 64 - l) // 2
    fr[:, t:t + hh, l:l + ww] = rng.integers(0, 256, (3, hh, ww, 3), dtype=np.uint8)
    fr = fr if ch == 3 else np.ascontiguousarray(fr[..., 1])
    check(gpu, fr, [0, 1, 3], want=[(t, l, hh, ww)] * 2)


# ---- 4. videos ----

def test_union_over_frames_an_empty_video_and_no_work(gpu, hvd):
    h, w = 100, 130
    a, b, c = base(h, w, 3, (5, 7, 64, 70)), base(h, w, 3, (20, 30, 70, 64)), base(h, w, 3, (30, 60, 40, 40))
    flat = np.full((h, w, 3), FLAT, np.uint8)
    frames = np.stack([a, b, c, flat, a])
    # video 0: the union of three boxes (the third, 40 x 40, would be too small alone); 1: empty; 2: flat; 3: a alone
    check(gpu, frames, [0, 3, 3, 4, 5], want=[(5, 7, 85, 93), (0, 0, 100, 130), (0, 0, 100, 130), (5, 7, 64, 70)])
    assert np.array_equal(hvd.vpdq.content_rects(frames, [0, 3, 3, 4, 5], detail=True),
                          D.rule_rects(frames, [0, 3, 3, 4, 5]))
    # V = 0 and n = 0 are no work
    lib = gpu.ensure()
    gpu.check(lib.hvd_dev_content_rects_detail(None, 0, h, w, 3, None, 0, 8, 8, None))
    assert device_rects(gpu, frames, [0, 0, 0], n=0).tolist() == [[0, 0, h, w]] * 2
    none = np.zeros((0, h, w, 3), np.uint8)
    assert hvd.vpdq.content_rects(none, [0], detail=True).shape == (0, 4)
    for level, count in ((-1, 8), (255, 8), (8, 0)):
        assert lib.hvd_dev_content_rects_detail(None, 0, h, w, 3, None, 0, level, count, None) == gpu.HVD_ERR_ARG


def video_of_frame(offsets, V, f):
    """The kernel's clamped search: always in [0, V)."""
    lo, hi = 0, V
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if offsets[mid] <= f:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("offsets", [[0, 5, 2, 3, 6], [4, 4, 1, 0, 0], [0, 1, 2, 3, 3], [9, 9, 9, 9, 9]])
def test_a_broken_csr_gives_wrong_rectangles_and_nothing_else(gpu, offsets):
    """6 frames, 4 videos, offsets that decrease, stop short or point past the frames: every frame folds into the video the
    clamped search gives it -- checked by the result alone; the offsets array itself is as long as a sound one."""
    h, w = 100, 130
    blocks = [(1, 1, 64, 64), (30, 60, 66, 64), (10, 20, 70, 80), (5, 5, 90, 120), (2, 50, 64, 70), (36, 66, 64, 64)]
    frames = np.stack([base(h, w, 3, blk) for blk in blocks])
    want = []
    for v in range(4):
        mine = [blocks[f] for f in range(6) if video_of_frame(offsets, 4, f) == v]
        if not mine:
            want.append([0, 0, h, w])
            continue
        t, l = min(m[0] for m in mine), min(m[1] for m in mine)
        b, r = max(m[0] + m[2] for m in mine), max(m[1] + m[3] for m in mine)
        want.append([t, l, b - t, r - l])
    assert device_rects(gpu, frames, offsets).tolist() == want


# ---- 5. end to end on the 30-video library of blurred and gradient copies ----

@pytest.fixture(scope="module")
def library(oracle):
    frames, offsets, rects, groups = D.library_30()
    cropped, quality = A.oracle_cropped(oracle, frames, offsets, rects)
    return frames, offsets, rects, groups, cropped, quality


def test_library_hashes_qualities_and_rectangles_equal_the_oracle_on_the_crops(gpu, hvd, library):
    frames, offsets, rects, groups, cropped, quality = library
    h, q, r = hvd.vpdq.hash_frames_autocrop(frames, offsets, detail=True)
    assert np.array_equal(r, rects) and np.array_equal(q, quality) and np.array_equal(h, cropped)
    assert np.array_equal(hvd.vpdq.content_rects(frames, offsets, detail=True, detail_level=8, min_detail=8), rects)
    assert np.array_equal(device_rects(gpu, frames, offsets), rects)
    green = np.ascontiguousarray(frames[:40, :, :, 1])
    assert np.array_equal(hvd.vpdq.content_rects(green, offsets[:6], detail=True), rects[:5])
    # the black rule sees none of these bars
    assert np.array_equal(hvd.vpdq.content_rects(frames[:40], offsets[:6]), [[0, 0, 512, 512]] * 5)


def test_library_duplicates_are_the_expected_pairs(gpu, hvd, library):
    frames, offsets, rects, groups, cropped, quality = library
    from hvd_amd.vpdqpy import Vpdq

    videos = [frames[offsets[v]:offsets[v + 1]] for v in range(30)]
    rule = {"detail": True}
    phashes = hvd.pipeline.hash_videos(videos, autocrop=rule)
    assert [p.bytes for p in phashes] == [cropped[offsets[v]:offsets[v + 1]][quality[offsets[v]:offsets[v + 1]] >= 31].tobytes()
                                          for v in range(30)]
    found = hvd.search.find_potential_duplicates(phashes, threshold=50)
    assert found == A.expected_pairs(groups) and len(found) == 60
    for v in (0, 1, 3):
        assert Vpdq.computeHash(videos[v], autocrop={"detail": True, "detail_level": 8, "min_detail": 8}).bytes == phashes[v].bytes
    black = hvd.search.find_potential_duplicates(hvd.pipeline.hash_videos(videos[:5], autocrop=True), threshold=50)
    assert black == []


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_video_hasher_in_batches_equals_the_array_form(gpu, hvd, library, batch):
    frames, offsets, rects, groups, cropped, quality = library
    for v in (0, 2, 8):  # an original, a blurred pillar, a gradient letterbox
        fr = frames[offsets[v]:offsets[v + 1]]
        hs = hvd.vpdq.VideoHasher(1, 512, 512, 0, batch_bytes=batch * 512 * 512 * 3, autocrop={"detail": True})
        for f in fr:
            hs.hash_frame(f.tobytes())
        got = hs.finish()
        wh, wq, wr = hvd.vpdq.hash_frames_autocrop(fr, detail=True)
        assert hs.rect == tuple(rects[v].tolist()) == tuple(wr[0].tolist())
        assert got.bytes == wh[wq >= 31].tobytes() == cropped[offsets[v]:offsets[v + 1]][quality[offsets[v]:offsets[v + 1]] >= 31].tobytes()


def test_video_hasher_gray_with_parameters_and_the_native_argument_check(gpu, hvd):
    rng = np.random.default_rng(9)
    fr = np.full((7, 100, 130), 60, np.uint8)
    fr[:, 10:80, 20:100] = rng.integers(0, 256, (7, 70, 80), dtype=np.uint8)
    fr[3, 5, 40:43] = (90, 60, 90)  # 4 pairs in row 5 of one frame
    for count, rect in ((4, (5, 20, 75, 80)), (5, (10, 20, 70, 80))):
        hs = hvd.vpdq.VideoHasher(1, 130, 100, 0, batch_bytes=2 * 100 * 130, autocrop={"detail": True, "detail_level": 20, "min_detail": count})
        for f in fr:
            hs.hash_frame(f.tobytes())
        got = hs.finish()
        wh, wq, wr = hvd.vpdq.hash_frames_autocrop(fr, detail=True, detail_level=20, min_detail=count)
        assert hs.rect == rect == tuple(wr[0].tolist()) == tuple(D.rule_rects(fr, None, 20, count)[0].tolist())
        assert got.bytes == wh[wq >= 31].tobytes()
    lib = gpu.ensure()
    hd = C.c_void_p()
    for level, count in ((-1, 8), (255, 8), (8, 0)):
        assert lib.hvd_hasher_create_autocrop_detail(130, 100, 1, 4, level, count, 0, C.byref(hd)) == gpu.HVD_ERR_ARG


def test_pipeline_on_device_returns_the_same_pairs(gpu, hvd, oracle, library):
    frames, offsets, rects, groups, cropped, quality = library
    want = oracle.match_videos(cropped, offsets, A.FRAME_TOLERANCE)
    d_fr = gpu.DeviceBuffer.from_array(frames)
    try:
        tm = {}
        pairs, recs, _ = hvd.dedupe_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, autocrop={"detail": True}, timings=tm)
        assert [tuple(p) for p in pairs.tolist()] == A.expected_pairs(groups) and len(pairs) == 60
        assert recs.dtype == want.dtype and np.array_equal(recs, want)
        assert tm["rects_ms"] > 0 and tm["hash_ms"] > 0
        d_h, d_q, d_r = hvd.pipeline.hash_frames_autocrop_on_device(d_fr.ptr, 240, 512, 512, 3, offsets, detail=True)
        try:
            assert np.array_equal(d_r.to_array(np.int32, 120).reshape(30, 4), rects)
            assert np.array_equal(d_h.to_array(np.uint8, 32 * 240).reshape(240, 32), cropped)
        finally:
            for b in (d_h, d_q, d_r):
                b.free()
    finally:
        d_fr.free()


def test_fma_dct_mode_once(gpu, hvd, oracle, library):
    frames, offsets, rects, groups, cropped, quality = library
    fr, off = frames[:24], offsets[:4]
    want_h, want_q = A.oracle_cropped(oracle, fr, off, rects[:3], fma=True)
    with dct_mode(hvd, "fma"):
        h, q, r = hvd.vpdq.hash_frames_autocrop(fr, off, detail=True)
    assert np.array_equal(r, rects[:3]) and np.array_equal(q, want_q) and np.array_equal(h, want_h)
