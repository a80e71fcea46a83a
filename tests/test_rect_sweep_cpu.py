"""The case list of the fused rectangle down-sampler's side-length sweep (tests/rect_sweep_helpers.py), checked on the CPU:
tests/test_gpu_rect_sweep.py runs exactly these rectangles, so what it can notice is what this list reaches. The conditions
below are requirements on the list, not measurements of it."""
import numpy as np
import pytest

import rect_sweep_helpers as S

SIDES = set(range(64, 513))


def test_full_last_strip_is_what_the_rule_gives():
    want = [ww for ww in range(64, 513) if S.window(ww) >> 1 >= 1 and (ww + (S.window(ww) >> 1)) % 32 == 0]
    assert tuple(want) == S.FULL_LAST_STRIP and len(want) == 12


def test_the_partner_map_is_a_permutation():
    assert sorted(S.partner(s) for s in SIDES) == sorted(SIDES)
    assert S.partner(64) == 64 and all(S.partner(s) != 64 for s in SIDES if s != 64)


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_pairing_holds_every_width_and_every_height(name):
    rects = S.pairing(name, 512, 512)
    assert {r[3] for r in rects} == SIDES and {r[2] for r in rects} == SIDES
    assert (64, 64) not in {r[2:] for r in rects}, "64 x 64 is k_luma64_rect's case"
    swept = [r[S.swept_axis(name)] for r in rects[:448]]
    assert swept == list(range(65, 513)), "the swept side runs through 65..512 in order"
    other = 5 - S.swept_axis(name)
    assert all(r[other] == S.partner(r[S.swept_axis(name)]) for r in rects[:448])


def test_the_squares():
    assert [r[2:] for r in S.pairing("C")] == [(s, s) for s in range(65, 513)]


def test_every_row_class_and_every_column_class():
    rects = S.pairing("A") + S.pairing("B")
    rows = {S.row_class(r[3]) for r in rects}
    cols = {S.col_class(r[2]) for r in rects}
    assert rows == {(wx, m) for wx in (1, 2, 3, 4) for m in range(32)} and len(rows) == 128
    assert cols == {(wy, m) for wy in (1, 2, 3, 4) for m in range(8)} and len(cols) == 32
    # ... and either pairing alone does, on the smaller frame as well but for the sides it cannot hold
    for name in "AB":
        assert {S.row_class(r[3]) for r in S.pairing(name)} == rows and {S.col_class(r[2]) for r in S.pairing(name)} == cols
        small = S.pairing(name, 511, 509)
        # (a pair goes with either of its sides: up to four widths and four heights below the frame's are lost that way)
        assert len(set(range(64, 510)) - {r[3] for r in small}) <= 4 and len(set(range(64, 512)) - {r[2] for r in small}) <= 4
        assert {S.row_class(r[3]) for r in small} == rows and {S.col_class(r[2]) for r in small} == cols


def test_every_full_last_strip_width_under_several_heights():
    rects = S.pairing("A") + S.pairing("B")
    for ww in S.FULL_LAST_STRIP:
        heights = {r[2] for r in rects if r[3] == ww}
        assert len(heights) >= 2 and len(heights - {64}) >= 2, (ww, heights)
    cases = S.full_last_strip_cases()
    assert {(r[2], r[3]) for r in cases} == {(hh, ww) for ww in S.FULL_LAST_STRIP for hh in (65, 257, 511)}
    assert all(r[0] + r[2] <= 512 and r[1] + r[3] <= 512 and min(r[:2]) >= 0 for r in cases)
    assert {S.lead(r, f, 512, 512, 3) for f, r in enumerate(cases)} == {0, 1, 2, 3}


def test_a_side_of_64_meets_many_partners():
    for name in "AB":
        rects = S.pairing(name)
        assert len({r[2] for r in rects if r[3] == 64 and r[2] != 64}) >= 16
        assert len({r[3] for r in rects if r[2] == 64 and r[3] != 64}) >= 16
        assert set(S.FULL_LAST_STRIP) <= {r[3] for r in rects if r[2] == 64}
        assert {hh % 8 for _, _, hh, ww in rects if ww == 64 and hh <= 128} == set(range(8))


@pytest.mark.parametrize("h,w", S.FRAMES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_every_rectangle_lies_inside_its_frame(name, h, w):
    rects = S.pairing(name, h, w)
    assert rects
    for top, left, hh, ww in rects:
        assert 0 <= top <= 3 and 0 <= left <= 3 and 64 <= hh and 64 <= ww and top + hh <= h and left + ww <= w
    fit = [(hh, ww) for hh, ww in S.sizes(name) if hh <= h and ww <= w]
    assert [r[2:] for r in rects] == fit, "only what does not fit is dropped"
    # the origins move wherever there is room
    roomy = [r for r in rects if r[0] + r[2] + 3 <= h and r[1] + r[3] + 3 <= w]
    assert {(r[0], r[1]) for r in roomy} == {(t, l) for t in range(4) for l in range(4)}


@pytest.mark.parametrize("h,w", S.FRAMES)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_launches(name, h, w):
    """One launch per window of the swept side: together the pairing, each small enough for the host's memory (one frame of
    up to 768 KiB per rectangle), and in each the first row of the rectangles starts at every byte of a 32-bit word."""
    groups = S.by_window(name, h, w)
    assert sorted(groups) == [1, 2, 3, 4]
    assert sorted(r for g in groups.values() for r in g) == sorted(S.pairing(name, h, w))
    for win, g in groups.items():
        assert 60 <= len(g) <= 140, (win, len(g))
        assert all(S.window(r[S.swept_axis(name)]) == win for r in g)
        for ch in (1, 3):
            assert {S.lead(r, f, h, w, ch) for f, r in enumerate(g)} == {0, 1, 2, 3}, (win, ch)


def test_rgb_leads_per_row_class():
    """On the 512-wide frame a row's first byte is at 3 * left mod 4. In pairing A every row class of the windows 2..4 (four
    widths each) meets all four, where the frame leaves the room; on the odd-width frame the later rows of any one rectangle do."""
    groups = S.by_window("A", 512, 512)
    for win in (2, 3, 4):
        seen = {}
        for f, r in enumerate(groups[win]):
            if r[2] != 64:
                seen.setdefault(S.row_class(r[3]), set()).add(S.lead(r, f, 512, 512, 3))
        assert len(seen) == 32 and all(len(v) >= 3 for v in seen.values()), win
        short = [k for k, v in seen.items() if len(v) < 4]
        assert short in ([], [(4, 31)]), "only next to width 511, which leaves one column of room, is a lead missing"
    r = S.pairing("A", 511, 509)[0]
    for ch in (1, 3):
        assert {S.lead(r, 0, 511, 509, ch, y) for y in range(4)} == {0, 1, 2, 3}


def test_samples_and_describe():
    assert [S.sample(j, 64) for j in range(64)] == list(range(64)), "a side of 64: a sample in every step"
    for length in (65, 255, 510, 512):
        s = [S.sample(j, length) for j in range(64)]
        assert s == sorted(set(s)) and s[0] >= S.window(length) - 1 and s[-1] <= length - S.window(length)
    text = S.describe((0, 1, 300, 255), 63, 63)
    assert "row_class (2, 31)" in text and "col_class (3, 4)" in text and "strip 7 " in text and "of 8 strips" in text


def test_differences_names_the_class_and_the_strip():
    """What the GPU test prints when a plane differs, on a made-up difference of one ulp in one cell."""
    rects = [(0, 0, 100, 200), (1, 2, 300, 255), (0, 0, 64, 70)]
    offsets = [0, 2, 3, 4]
    want = np.random.default_rng(1).random((4, 64, 64), dtype=np.float32)
    assert S.differences(want.copy(), want, offsets, rects) == ["0 of 4 planes differ from the oracle's"]
    got = want.copy()
    got[2, 63, 63] = np.nextafter(got[2, 63, 63], np.float32(2))
    lines = S.differences(got, want, offsets, rects)
    assert lines[0].startswith("1 of 4 planes") and len(lines) == 4
    assert "frame 2: 1 cells" in lines[1] and "rect (1, 2, 300, 255) row_class (2, 31) col_class (3, 4)" in lines[1]
    assert "strip 7 column 31 of 8 strips" in lines[1] and lines[2].strip() == "row classes [(2, 31)]"
    got[0, 0, 0] = -got[0, 0, 0] - 1
    assert "row classes [(2, 8), (2, 31)]" in S.differences(got, want, offsets, rects)[-2]
    assert np.array_equal(want, np.float32(-0.0) + want) and S.differences(-np.zeros((1, 64, 64), np.float32), np.zeros(
        (1, 64, 64), np.float32), [0, 1], rects[:1])[0].startswith("1 of 1"), "bits, not values: -0.0 is not 0.0"


@pytest.mark.parametrize("h,w", [(512, 512), (500, 508)])
def test_crop_calls(h, w):
    calls = S.crop_calls(h, w)
    fit = [r for r in S.pairing("A", h, w) if 64 not in r[2:]]
    flat = [r for c in calls for r in c if 64 not in r[2:]]
    assert sorted(flat) == sorted(fit), "every rectangle of pairing A that fits and has no side of 64, once"
    assert all(r in S.pairing("A", h, w) for c in calls for r in c if r[2:] != (64, 64))
    widths = {r[3] for c in calls for r in c}
    if (h, w) == (512, 512):
        assert widths == set(range(64, 513)), "every width"
    else:  # (a width goes with its height: the partners of the heights above the frame's are lost)
        assert len(set(range(64, w + 1)) - widths) <= 512 - h
    assert {S.row_class(x) for x in widths} == {(wx, m) for wx in (1, 2, 3, 4) for m in range(32)}
    positions = set()
    falling = rising = 0
    steps = {(a, b): 0 for a in (-1, 1) for b in (-1, 1)}  # (height, width) shrinks / grows from one rectangle to the next
    for c, call in enumerate(calls):
        assert len(call) == S.MAX_CROPS
        small = [k for k, r in enumerate(call) if r[2:] == (64, 64)]
        assert len(small) == 1
        positions.add(small[0])
        for top, left, hh, ww in call:
            assert top >= 0 and left >= 0 and hh >= 64 and ww >= 64 and top + hh <= h and left + ww <= w
        areas = [r[2] * r[3] for r in call if r[2:] != (64, 64)]
        assert areas == sorted(areas, reverse=c % 2 == 0)
        falling += c % 2 == 0
        rising += c % 2 == 1
        assert len({S.window(r[3]) for r in call}) == 4, "a call mixes the row windows"
        body = [r for r in call if r[2:] != (64, 64)]
        for a, b in zip(body, body[1:]):
            if a[2] != b[2]:
                steps[(1 if b[2] > a[2] else -1, 1 if b[3] > a[3] else -1)] += 1
    assert positions == set(range(S.MAX_CROPS)) and abs(falling - rising) <= 1
    # a rectangle follows one that left more rows, more columns, or both in the LDS, and the other way round
    assert min(steps.values()) >= 15, steps


def test_the_oracle_notices_a_shift_by_one(oracle):
    """Noise makes every pixel count: the plane of the crop one column to the right, or one row down, is another plane, at
    every window and at both ends of the range. (On a flat frame none of these would differ, and the sweep would prove
    nothing about where a rectangle starts.)"""
    rng = np.random.default_rng(5)
    gray = rng.integers(0, 256, (1, 512, 512), dtype=np.uint8)
    rgb = rng.integers(0, 256, (1, 512, 512, 3), dtype=np.uint8)
    for hh, ww in [(65, 64), (64, 65), (100, 128), (129, 255), (300, 383), (511, 510), (257, 414), (511, 511)]:
        for fr in (gray, rgb):
            crop = lambda t, l: oracle.planes64(fr[:, t:t + hh, l:l + ww])
            base = crop(0, 0)
            assert np.array_equal(base, crop(0, 0))
            right, down = crop(0, 1), crop(1, 0)
            # not one cell here and there: most of the plane moves
            assert (right != base).mean() > 0.9 and (down != base).mean() > 0.9, (hh, ww)
            assert (right != down).mean() > 0.9
