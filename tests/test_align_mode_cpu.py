"""The alignment mode without a GPU: search.ALIGN_ROWS names, for each of the four alignments, entries that exist
with the record and scratch sizes the header gives, and the one fold behind the four *_excerpts_from_records functions degenerates
as their docstrings say -- a single-line record reads as a record of one segment, a slope-one record as one at rate (1, 1).
Asserted elsewhere and not repeated here: each fold on hand-made records of its own kind (test_align_cpu, test_segments_cpu,
test_rates_cpu, test_rate_segments_cpu: orientation, floor, threshold edge, INT32_MIN), the same degenerations on whole searches
through a matcher (test_rates_cpu and test_rate_segments_cpu, "search on the reference matcher"), and the call transcript of
DeviceLibrary.align (test_pipeline_calls_cpu)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

INT32_MIN = -(1 << 31)
LENGTHS = [10, 20, 10, 0, 8]  # 0 and 2 tie; 3 is empty; 4 of 8 frames is min_aligned and exactly 50 %


def test_table_rows(hvd):
    from hvd_amd import _lib, pipeline, search

    lib = _lib.load()  # (no hvd_init: the scratch-size entries need no device)
    assert sorted(search.ALIGN_ROWS) == [(False, False), (False, True), (True, False), (True, True)]
    for mode, size, runs in ((search.AlignMode(), 48, 1), (search.AlignMode(None, 8), 288, 2),
                             (search.AlignMode(((1, 1),)), 64, 1), (search.AlignMode(((1, 1),), 8), 416, 2)):
        row = mode.row
        assert row is search.ALIGN_ROWS[mode.rates is not None, mode.max_segments is not None]
        for name in (row.host_entry, row.device_entry, row.scratch_entry):
            assert name in _lib.SIGNATURES, name
        assert row.dtype.itemsize == size
        assert callable(getattr(search, row.method)) and callable(getattr(pipeline.DeviceLibrary, row.method.replace("_videos", "")))
        sb = C.c_size_t(1)
        assert getattr(lib, row.scratch_entry)(7202, C.byref(sb)) == _lib.HVD_OK and sb.value == 64 * 4 * (7202 + runs * (225 + 3))
        assert getattr(lib, row.scratch_entry)(4096, C.byref(sb)) == _lib.HVD_OK and sb.value == 0
        # what the C entries take between slack and the scratch: the list, then the limits
        rates = None if mode.rates is None else search.rate_array(mode.rates)
        extra = len(_lib.SIGNATURES[row.host_entry][1]) - len(_lib.SIGNATURES["hvd_vpdq_align_videos"][1])
        assert len(mode.entry_args(rates)) == extra == len(_lib.SIGNATURES[row.device_entry][1]) - \
            len(_lib.SIGNATURES["hvd_dev_vpdq_align_videos"][1])


def slope_one_records():
    """VALIGN records over LENGTHS: every orientation (a short, b short, the tie both ways, the 8-frame video on either side) with
    3..6 aligned frames of the short video -- one below min_aligned = 4, at it, and 40 / 50 / 60 % of ten frames, 37.5 / 50 % of
    eight -- then an INT32_MIN record that would otherwise be kept, and the empty video on either side."""
    from hvd_amd._lib import VALIGN_DTYPE

    recs = []
    for a, b in ((0, 1), (1, 0), (0, 2), (2, 0), (4, 1), (1, 4)):
        a_short = LENGTHS[a] <= LENGTHS[b]
        for on in (3, 4, 5, 6):
            k = len(recs)
            q_on, t_on = (on, on + 1) if a_short else (on + 2, on)
            # a, b, q_hits, t_hits, offset, band_votes, q_aligned, t_aligned, q_first, q_last, t_first, t_last
            recs.append((a, b, q_on + 1, t_on + 1, (-1) ** k * (k + 1), on + 3, q_on, t_on, k % 3, k % 3 + q_on, k % 4 + 1, k % 4 + t_on + 2))
    recs.append((0, 1, 9, 9, INT32_MIN, 9, 9, 9, 0, 8, 5, 13))
    recs.append((3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    recs.append((1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    return np.array(recs, dtype=VALIGN_DTYPE)


def as_rates(recs, num=1, den=1, index=0):
    from hvd_amd._lib import VALIGN_DTYPE, VRATE_DTYPE

    out = np.zeros(len(recs), dtype=VRATE_DTYPE)
    for f in VALIGN_DTYPE.names:
        out[f] = recs[f]
    out["rate_num"], out["rate_den"], out["rate_index"] = num, den, index
    return out


def as_segments(recs, dtype):
    """One-segment records of `dtype` (VSEGMENTS or VRSEGMENTS) out of single-line records: n_segments 1, the line in seg[0]; a
    pair that could not be aligned keeps n_segments 0 and INT32_MIN in seg[0].offset, an empty one the zero record."""
    out = np.zeros(len(recs), dtype=dtype)
    for f in ("a", "b", "q_hits", "t_hits"):
        out[f] = recs[f]
    lost, none = recs["offset"] == INT32_MIN, recs["q_hits"] == 0
    out["n_segments"] = np.where(lost | none, 0, 1)
    out["q_covered"], out["t_covered"] = recs["q_aligned"], recs["t_aligned"]
    for f in dtype["seg"].base.names:
        if f in recs.dtype.names:
            out["seg"][f][:, 0] = recs[f]
    return out


@pytest.mark.parametrize("threshold,min_aligned,kept", [(50.0, 4, 14), (30.0, 4, 18), (30.0, 3, 24), (60.0, 4, 8)])
def test_fold_degenerations(hvd, threshold, min_aligned, kept):
    from hvd_amd import search
    from hvd_amd._lib import VRSEGMENTS_DTYPE, VSEGMENTS_DTYPE

    recs = slope_one_records()
    sim = np.arange(len(recs), dtype=np.float64)
    args = (LENGTHS, sim, threshold, min_aligned)
    plain = search.excerpts_from_records(recs, *args)
    # the count, by hand: per orientation the `on` values that pass both the floor and int(100 on / n_short) >= threshold
    assert len(plain) == kept and all(type(e.offset) is int for e in plain)
    assert not any((e.short, e.long) in ((3, 1), (1, 3)) for e in plain)
    assert not any(e.similarity == float(len(recs) - 3) for e in plain)  # the INT32_MIN record
    short_of = {(int(r["a"]), int(r["b"])) if LENGTHS[r["a"]] <= LENGTHS[r["b"]] else (int(r["b"]), int(r["a"])) for r in recs}
    assert {(e.short, e.long) for e in plain} <= short_of and (0, 2) in short_of and (2, 0) in short_of  # a on a tie

    rated = search.rate_excerpts_from_records(as_rates(recs), *args)
    assert [(r.short, r.long, r.offset, r.first, r.last, r.coverage, r.similarity) for r in rated] == [tuple(e) for e in plain]
    assert all(r.rate == 1 and type(r.rate) is Fraction and type(r.offset) is Fraction for r in rated)

    by_sim = {int(s): r for s, r in zip(sim, recs)}
    segmented = search.segmented_excerpts_from_records(as_segments(recs, VSEGMENTS_DTYPE), *args)
    both = search.rate_segmented_excerpts_from_records(as_segments(as_rates(recs), VRSEGMENTS_DTYPE), *args)
    assert len(segmented) == len(both) == len(plain) and segmented == sorted(segmented) and both == sorted(both)
    # (one-line excerpts sort by offset after the pair, segmented ones by coverage: paired here by the record they came from)
    of_record = lambda found: sorted(found, key=lambda x: x.similarity)  # noqa: E731
    for e, s, rs in zip(of_record(plain), of_record(segmented), of_record(both)):
        assert (s.short, s.long, s.coverage, s.similarity) == (e.short, e.long, e.coverage, e.similarity) == rs[:4]
        r = by_sim[int(e.similarity)]
        side = "q" if e.short == r["a"] else "t"
        want = search.Segment(e.offset, int(r[side + "_first"]), int(r[side + "_last"]), e.first, e.last, int(r[side + "_aligned"]))
        assert s.segments == (want,) and type(s.segments[0].offset) is int
        assert rs.segments == (search.RateSegment(Fraction(1), Fraction(e.offset), *want[1:]),)
        assert e.coverage == 100.0 * want.aligned / LENGTHS[e.short]


def test_a_rate_with_b_short_by_hand(hvd):
    """A record (num, den, d) = (3, 2, 7) reads p_b = 3/2 p_a + 7/2; with b short that is p_a = 2/3 p_b - 7/3, and first / last
    are a's."""
    from hvd_amd import search
    from hvd_amd._lib import VALIGN_DTYPE, VRSEGMENTS_DTYPE

    rec = np.array([(1, 0, 9, 8, 7, 11, 9, 8, 2, 6, 10, 19)], dtype=VALIGN_DTYPE)  # a = the 20-frame video: b is short
    got = search.rate_excerpts_from_records(as_rates(rec, 3, 2, 5), LENGTHS, [12.5])
    assert got == [search.RateExcerpt(0, 1, Fraction(2, 3), Fraction(-7, 3), 2, 6, 80.0, 12.5)]
    got = search.rate_segmented_excerpts_from_records(as_segments(as_rates(rec, 3, 2, 5), VRSEGMENTS_DTYPE), LENGTHS, [12.5])
    assert got == [search.RateSegmentedExcerpt(0, 1, 80.0, 12.5, (search.RateSegment(Fraction(2, 3), Fraction(-7, 3), 10, 19, 2, 6, 8),))]
    # and with a short, as it stands: the same words under pair (0, 1)
    rec["a"], rec["b"] = 0, 1
    got = search.rate_excerpts_from_records(as_rates(rec, 3, 2, 5), LENGTHS, [12.5])
    assert got == [search.RateExcerpt(0, 1, Fraction(3, 2), Fraction(7, 2), 10, 19, 90.0, 12.5)]
