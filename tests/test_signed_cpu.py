"""Time alignment with negative rates without a GPU: the numpy restatement of the rule (tests/signed_helpers.py)
gives the records of the table the feature was proposed on -- a reversed clip, a reversed 3/2 clip, a reel with reversed pieces,
none of which the forward lists report -- and has the four consequences the header states; list soundness; the host entry refuses
a broken list before it asks for a device and the existing entries keep refusing a negative num; the header, the dtypes, the
fold and the search on the reference matcher; the new kernel file has the shape of its siblings and compiles for gfx950 inside
their budget."""
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import rate_segments_helpers as RS
import rates_helpers as RH
import segments_helpers as SH
import signed_helpers as SG
from conftest import ROOT
from test_code_shape import HIPCC, LDS_PER_CU, _compile, waves_per_simd

CSRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
HEAD = ("a", "b", "q_hits", "t_hits", "n_segments", "q_covered", "t_covered", "reserved")


def words(segs):
    """(rate, offset, band_votes, q_aligned, t_aligned) of every segment."""
    return [((s[8], s[9]), s[0], s[1], s[2], s[3]) for s in segs]


# ---- the table ----

def test_reversed_clip_is_dropped_forward_and_whole_backward():
    t = SG.table()
    source, rev = t["source"], t["rev"]
    assert len(source) == 600 and len(rev) == 60
    line = RH.rates_pair(rev, source, rates=((1, 1),))
    assert line[3] == 2 and line[4] == 2  # the best forward band holds 2 hits: 2 of 60 aligned
    assert SH.segments_of_pair(rev, source, min_band_votes=4)[2] == []
    low = SH.segments_of_pair(rev, source, min_band_votes=1)[2]
    assert [s[2] for s in low] == [2] * 8 and sum(s[2] for s in low) == 16
    q_hits, t_hits, segs = SG.signed_pair(rev, source)
    assert (q_hits, t_hits) == (60, 60) and segs == [(159, 60, 60, 60, 0, 59, 100, 159, -1, 1, 1, 0)]
    # the same pair with the source as a
    assert SG.signed_pair(source, rev)[2] == [(159, 60, 60, 60, 100, 159, 0, 59, -1, 1, 1, 0)]


def test_reversed_clip_at_three_halves():
    t = SG.table()
    assert SG.LIST_32[7] == (-3, 2) and SG.sound_signed(SG.LIST_32)
    assert SG.signed_pair(t["rev32"], t["source"], rates=SG.LIST_32)[2] == [(600, 40, 40, 40, 0, 39, 242, 300, -3, 2, 7, 0)]


def test_reel_with_reversed_pieces():
    t = SG.table()
    reel, source = t["reel"], t["source"]
    assert len(reel) == 110
    fwd = RS.rate_segments_pair(reel, source, rates=((1, 1), (2, 1)), min_band_votes=4)[2]
    assert [(s[8:10], s[2]) for s in fwd] == [((1, 1), 40)]  # one segment, 40 of 110
    q_hits, t_hits, segs = SG.signed_pair(reel, source, rates=SG.FOUR_RATES, min_band_votes=4)
    assert words(segs) == [((1, 1), 50, 40, 40, 40), ((-1, 1), 479, 40, 40, 40), ((-2, 1), 460, 30, 30, 30)]
    assert sum(s[2] for s in segs) == 110 == q_hits


def test_shuffled_frames_stay_unreported():
    """Order still matters: the best band of 60 shuffled frames holds a handful of hits. (The proposal's table says 7 for its
    own shuffle; this library's, drawn after the reel from the same generator, gives 8.)"""
    t = SG.table()
    segs = SG.signed_pair(t["shuffled"], t["source"])[2]
    assert segs[0][1] == 8 and 100 * segs[0][2] // 60 < 50


def test_ping_pong_loop_keeps_one_half():
    """Out of scope: a clip forward, then the same frames backwards. The taken set gives the source's frames to the
    first half."""
    source = SG.table()["source"]
    loop = np.concatenate([source[100:160], source[100:160][::-1]])
    q_hits, t_hits, segs = SG.signed_pair(loop, source, min_band_votes=4)
    assert (q_hits, t_hits) == (120, 60) and segs == [(100, 61, 61, 60, 0, 60, 100, 159, 1, 1, 0, 0)]


# ---- corner bins ----

def corner_pair():
    rng = np.random.default_rng(77)
    a, b = RH._rand(rng, 30), RH._rand(rng, 50)
    a[0], a[29] = b[0], b[49]
    return a, b


def test_corner_bins_under_a_reversed_rate():
    """Two hits, in the first and in the last core bin of the histogram at (-1, 1): the smallest delta is p_b0 + p_a0, the
    largest p_b1 + p_a1. A dmin built from p_a1 loses the first."""
    a, b = corner_pair()
    pa, pb = np.arange(30) + 7, np.arange(50) + 11
    q_hits, t_hits, segs = SG.signed_pair(a, b, pa, pb, rates=((-1, 1),), max_segments=2)
    assert (q_hits, t_hits) == (2, 2)
    assert segs == [(18, 1, 1, 1, 7, 7, 11, 11, -1, 1, 0, 0), (96, 1, 1, 1, 36, 36, 60, 60, -1, 1, 0, 0)]
    assert SG.bins_of(29, 49, ((-1, 1),), 1) == 81 and 96 - 18 == 29 + 49


# ---- the four consequences ----

@pytest.fixture(scope="module")
def libraries():
    out = []
    for source, reel in (RS.reel_b(), RS.reel_c()):
        frames, offsets = RH.join([reel, source])
        out.append((frames, offsets, [(0, 1), (1, 0)]))
    frames, offsets = RH.join(RH.mixed_library(73))
    V = len(offsets) - 1
    out.append((frames, offsets, [(a, b) for a in range(V) for b in range(V)]))
    return out


def test_a_forward_lists_degenerate(libraries):
    for frames, offsets, pairs in libraries:
        for K, floor in ((8, 1), (8, 4), (1, 1)):
            got = SG.align_signed(frames, offsets, pairs, None, RH.DEFAULT_RATES, max_segments=K, min_band_votes=floor)
            SG.same_words(got, RS.align_rate_segments(frames, offsets, pairs, None, RH.DEFAULT_RATES, max_segments=K, min_band_votes=floor))
        line = RH.align_rates(frames, offsets, pairs)
        for g, r in zip(got, line):  # max_segments = 1: seg[0] is the rate alignment's record
            assert g.tolist()[:4] == r.tolist()[:4] and g["seg"][0].tolist() == r.tolist()[4:]


def test_b_hit_counts_are_list_free(libraries):
    frames, offsets, pairs = SG.table_library()
    lists = (SG.REVERSED_RATES, SG.FOUR_RATES, ((-1, 1),), SG.LIST_32, ((1, 1),))
    base = RS.align_rate_segments(frames, offsets, pairs, None, ((1, 1),))
    for rates in lists:
        for K in (1, 8):
            got = SG.align_signed(frames, offsets, pairs, None, rates, max_segments=K)
            assert np.array_equal(got["q_hits"], base["q_hits"]) and np.array_equal(got["t_hits"], base["t_hits"])


def test_c_ties_go_forward_by_list_order():
    rng = np.random.default_rng(78)
    h = RH._rand(rng, 1)
    A, B = np.repeat(h, 50, axis=0), np.repeat(h, 80, axis=0)
    assert SG.signed_pair(A, B, max_segments=1)[2] == [(1, 150, 50, 52, 0, 49, 0, 51, 1, 1, 0, 0)]
    assert SG.signed_pair(A, B, rates=((-1, 1), (1, 1)), max_segments=1)[2] == [(50, 150, 50, 52, 0, 49, 0, 51, -1, 1, 0, 0)]
    # one hit
    a, b = RH._rand(rng, 9), RH._rand(rng, 12)
    a[4] = b[7]
    assert SG.signed_pair(a, b)[2] == [(3, 1, 1, 1, 4, 4, 7, 7, 1, 1, 0, 0)]
    assert SG.signed_pair(a, b, rates=((-1, 1), (1, 1)))[2] == [(11, 1, 1, 1, 4, 4, 7, 7, -1, 1, 0, 0)]


def test_d_reflection():
    """Reversing a's frame order and negating every num: the same band_votes, q_aligned, t_aligned, t_first, t_last per segment,
    offset' = offset + num (n_a - 1), q_first' = n_a - 1 - q_last -- on pairs without a tie on |d|. The one check of the
    restatement that does not come from the restatement."""
    t = SG.table()
    vids, _ = SG.planted_signed(79)
    cases = [(t["rev"], t["source"], SG.REVERSED_RATES), (t["source"], t["rev"], SG.REVERSED_RATES),
             (t["rev32"], t["source"], SG.LIST_32), (t["reel"], t["source"], SG.FOUR_RATES), (t["source"], t["reel"], SG.FOUR_RATES)]
    cases += [(vids[v], vids[0], SG.WIDE_SIGNED) for v in range(1, 9)] + [(vids[0], vids[v], SG.WIDE_SIGNED) for v in range(1, 9)]
    cases += [(RS.reel_b()[1], RS.reel_b()[0], RH.DEFAULT_RATES), (RS.reel_c()[1], RS.reel_c()[0], RH.DEFAULT_RATES)]
    checked = 0
    for A, B, rates in cases:
        for floor in (1, 4):
            if not SG.no_tie_on_d(A, B, rates=rates, min_band_votes=floor):
                continue
            n_a = len(A)
            q_hits, t_hits, segs = SG.signed_pair(A, B, rates=rates, min_band_votes=floor)
            q2, t2, mirrored = SG.signed_pair(A[::-1], B, rates=SG.flipped(rates), min_band_votes=floor)
            assert (q_hits, t_hits) == (q2, t2) and len(segs) == len(mirrored)
            checked += len(segs) >= 1  # (a floor of 4 leaves the sparse clips -- one frame in eight -- without a segment)
            for s, m in zip(segs, mirrored):
                assert m[0] == s[0] + s[8] * (n_a - 1)
                assert m[1:4] == s[1:4] and m[6:8] == s[6:8] and m[4] == n_a - 1 - s[5] and m[5] == n_a - 1 - s[4]
                assert m[8:] == (-s[8],) + s[9:]
    assert checked >= 12


# ---- list soundness ----

def test_list_soundness():
    assert SG.sound_signed(SG.REVERSED_RATES) and SG.sound_signed(SG.FOUR_RATES) and SG.sound_signed(SG.WIDE_SIGNED)
    assert SG.sound_signed(((-8, 1),)) and SG.sound_signed(RH.DEFAULT_RATES)
    assert len(SG.BROKEN_LISTS) == 7 and len(SG.BROKEN_LISTS[5]) == 9
    for bad in SG.BROKEN_LISTS:
        assert not SG.sound_signed(bad), bad
    rng = np.random.default_rng(80)
    frames, offsets = RH.join([RH._rand(rng, 5), RH._rand(rng, 7)])
    for bad in SG.BROKEN_LISTS:
        assert SG.align_signed(frames, offsets, [(0, 1)], rates=bad)[0] == SG.lost_record(0, 1)


def test_host_entries_and_broken_lists_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()  # (no hvd_init here: a sound call's answer depends on the library's state, none is made)
    rng = np.random.default_rng(81)
    frames, offsets = RH.join([RH._rand(rng, 5), RH._rand(rng, 7)])
    out = np.zeros(1, dtype=SG.VSSEGMENTS_DTYPE)

    def call(entry, rates, n_rates=None, max_segments=8, min_band_votes=1, pair=(0, 1), positions=None):
        r = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
        pairs = np.array([pair], dtype=np.uint32)
        pos = None if positions is None else positions.ctypes.data
        return getattr(lib, entry)(frames.ctypes.data, offsets.ctypes.data, 2, pos, frames.ctypes.data, offsets.ctypes.data, 2, pos,
                                   pairs.ctypes.data, 1, 31, 1, r.ctypes.data if r.size else None,
                                   len(r) if n_rates is None else n_rates, max_segments, min_band_votes, out.ctypes.data)

    for bad in SG.BROKEN_LISTS:
        assert call("hvd_vpdq_align_signed", bad) == _lib.HVD_ERR_ARG, bad
        assert "rates" in _lib.last_error()
    assert call("hvd_vpdq_align_signed", SG.REVERSED_RATES, n_rates=0) == _lib.HVD_ERR_ARG
    assert call("hvd_vpdq_align_signed", SG.REVERSED_RATES, n_rates=9) == _lib.HVD_ERR_ARG
    # everything hvd_vpdq_align_rate_segments rejects
    for k in (0, 9, -1):
        assert call("hvd_vpdq_align_signed", SG.REVERSED_RATES, max_segments=k) == _lib.HVD_ERR_ARG and "max_segments" in _lib.last_error()
    assert call("hvd_vpdq_align_signed", SG.REVERSED_RATES, min_band_votes=0) == _lib.HVD_ERR_ARG
    assert call("hvd_vpdq_align_signed", SG.REVERSED_RATES, pair=(0, 2)) == _lib.HVD_ERR_ARG and "outside" in _lib.last_error()
    positions = np.concatenate([np.arange(5), np.arange(6), [131071]]).astype(np.int32)
    assert call("hvd_vpdq_align_signed", [(1, 1), (-1, 8)], positions=positions) == _lib.HVD_ERR_ARG and "2^20" in _lib.last_error()
    assert call("hvd_vpdq_align_signed", [(1, 1), (-8, 1)], pair=(1, 0), positions=positions) == _lib.HVD_ERR_ARG and "2^20" in _lib.last_error()
    # the existing entries keep rejecting a negative num
    assert call("hvd_vpdq_align_rate_segments", ((-1, 1),)) == _lib.HVD_ERR_ARG and "rates" in _lib.last_error()
    assert call("hvd_vpdq_align_rate_segments", SG.REVERSED_RATES) == _lib.HVD_ERR_ARG
    assert not out.view(np.uint32).any()
    import ctypes as C
    sb, sb2 = C.c_size_t(1), C.c_size_t(2)
    for bins in (0, 4096, 4161, 7202, 1 << 20):
        assert lib.hvd_signed_scratch_bytes(bins, C.byref(sb)) == _lib.HVD_OK
        assert lib.hvd_rate_segments_scratch_bytes(bins, C.byref(sb2)) == _lib.HVD_OK and sb.value == sb2.value
    assert lib.hvd_signed_scratch_bytes(4161, C.byref(sb)) == _lib.HVD_OK and sb.value == 64 * 4 * (4161 + 2 * (130 + 3))
    assert lib.hvd_signed_scratch_bytes((1 << 20) + 1, C.byref(sb)) == _lib.HVD_ERR_ARG


# ---- surface shape ----

def test_header_dtypes_and_surfaces(hvd):
    from hvd_amd import _lib, pipeline, search

    assert _lib.VSSEGMENT_DTYPE == SG.VSSEGMENT_DTYPE and _lib.VSSEGMENT_DTYPE.itemsize == 48
    assert _lib.VSSEGMENTS_DTYPE == SG.VSSEGMENTS_DTYPE and _lib.VSSEGMENTS_DTYPE.itemsize == 416
    assert _lib.VSSEGMENT_DTYPE.names == _lib.VRSEGMENT_DTYPE.names and _lib.VSSEGMENT_DTYPE["rate_num"] == np.dtype("<i4")
    assert [_lib.VSSEGMENT_DTYPE[n] for n in _lib.VSSEGMENT_DTYPE.names if n != "rate_num"] == [
        _lib.VRSEGMENT_DTYPE[n] for n in _lib.VRSEGMENT_DTYPE.names if n != "rate_num"]
    assert _lib.VSSEGMENTS_DTYPE.names[:8] == HEAD and _lib.VSSEGMENTS_DTYPE.fields["seg"][1] == 32
    hdr = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert "#define HVD_ABI_VERSION 6 " in hdr
    seg = re.search(r"typedef struct hvd_vssegment \{(.*?)\} hvd_vssegment;", hdr, re.S).group(1)
    assert "int32_t rate_num;" in seg and "uint32_t rate_den, rate_index, reserved;" in seg
    for struct, dtype in (("hvd_vssegment", _lib.VSSEGMENT_DTYPE), ("hvd_vssegments", _lib.VSSEGMENTS_DTYPE)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, re.S).group(1)
        names = tuple(n.strip() for d in body.split(";") if d.strip() for n in d.split(None, 1)[1].split(","))
        assert names == (dtype.names[:-1] + ("seg[HVD_ALIGN_MAX_SEGMENTS]",) if struct.endswith("s") else dtype.names)
    abi = re.search(r"#define HVD_ABI_VERSION 6 /\*(.*?)\*/", hdr).group(1)
    for name, twin in (("hvd_vpdq_align_signed", "hvd_vpdq_align_rate_segments"), ("hvd_dev_vpdq_align_signed", "hvd_dev_vpdq_align_rate_segments"),
                       ("hvd_signed_scratch_bytes", "hvd_rate_segments_scratch_bytes")):
        assert re.search(rf"\bint {name}\(", hdr) and name in abi
        n_args = len(re.search(rf"\bint {name}\((.*?)\);", hdr, re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) and _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    assert sorted(search.ALIGN_ROWS) == [(False, False), (False, True), (True, False), (True, True)]
    mode = search.AlignMode(search.REVERSED_RATES, 8, 1, True)
    assert search.AlignMode._fields == ("rates", "max_segments", "min_band_votes", "signed") and search.AlignMode().signed is False
    assert mode.row is search.SIGNED_ROW and search.SIGNED_ROW not in search.ALIGN_ROWS.values()
    assert search.AlignMode(search.REVERSED_RATES, 8).row is search.ALIGN_ROWS[True, True]
    row = search.SIGNED_ROW
    assert row.dtype == _lib.VSSEGMENTS_DTYPE and row.method == "align_signed" and callable(getattr(search, row.method))
    assert (row.host_entry, row.device_entry, row.scratch_entry) == ("hvd_vpdq_align_signed", "hvd_dev_vpdq_align_signed",
                                                                      "hvd_signed_scratch_bytes")
    assert (row.excerpt, row.segment) == (search.RateSegmentedExcerpt, search.RateSegment)
    assert search.REVERSED_RATES == ((1, 1), (-1, 1)) == SG.REVERSED_RATES
    assert hvd.find_reversed_excerpts is search.find_reversed_excerpts
    assert callable(pipeline.find_reversed_excerpts_on_device) and callable(pipeline.DeviceLibrary.align_signed)
    assert callable(hvd.Vpdq.align_signed)


def made_record(a, b, segs):
    """segs: (offset, q_aligned, t_aligned, (q_first, q_last), (t_first, t_last), (num, den), index)."""
    full = [(d, max(qa, ta), qa, ta) + qs + ts + rate + (index, 0) for d, qa, ta, qs, ts, rate, index in segs]
    return SG.record(a, b, sum(s[2] for s in full), sum(s[3] for s in full), full)


def test_fold_reads_negative_rates_in_both_orientations(hvd):
    from hvd_amd import search

    RSeg, RSE = search.RateSegment, search.RateSegmentedExcerpt
    lengths = [60, 600, 40]
    recs = np.array([
        # a is short: p_b = -p_a + 159, and a forward piece p_b = p_a + 300
        made_record(0, 1, [(159, 30, 30, (0, 29), (130, 159), (-1, 1), 1), (300, 20, 20, (40, 59), (340, 359), (1, 1), 0)]),
        # b is short: d = 2 p_b + 3 p_a = 600, so p_a = -2/3 p_b + 200
        made_record(1, 2, [(600, 27, 40, (174, 200), (0, 39), (-3, 2), 7)]),
        SG.lost_record(0, 2),
    ], dtype=SG.VSSEGMENTS_DTYPE)
    got = search.signed_excerpts_from_records(recs, lengths, np.array([1.0, 2.0, 3.0]))
    assert got == [
        RSE(0, 1, 250.0 / 3.0, 1.0, (RSeg(Fraction(-1), Fraction(159), 0, 29, 130, 159, 30), RSeg(Fraction(1), Fraction(300), 40, 59, 340, 359, 20))),
        RSE(2, 1, 100.0, 2.0, (RSeg(Fraction(-2, 3), Fraction(200), 0, 39, 174, 200, 40),))]
    assert search._line_in_long(-3, 2, 600, True) == (Fraction(-3, 2), Fraction(300))
    assert search._line_in_long(-3, 2, 600, False) == (Fraction(-2, 3), Fraction(200))
    odd = recs.copy()
    odd[0]["seg"][0]["offset"] = SG.INT32_MIN
    assert [(e.short, e.long) for e in search.signed_excerpts_from_records(odd, lengths, np.zeros(3))] == [(2, 1)]


def test_search_on_the_reference_matcher(hvd):
    """The reversed clip and the reel are found by the new search, with negative rates, and by the forward search not; an
    all-positive list is the forward search."""
    from hvd_amd import search

    t = SG.table()
    rng = np.random.default_rng(82)
    vids = [t["rev"], t["reel"], t["source"], RH._rand(rng, 30)]  # (a clip ahead of its source is the a side of its pair)
    blobs = [v.tobytes() for v in vids]
    got = search.signed_excerpt_pairs(blobs, rates=SG.FOUR_RATES, matcher=SG.ReferenceMatcher)
    by = {(e.short, e.long): e for e in got}
    assert sorted(by) == [(0, 2), (1, 2)]
    assert by[(0, 2)].coverage == 100.0 and [tuple(s) for s in by[(0, 2)].segments] == [(-1, 159, 0, 59, 100, 159, 60)]
    assert by[(1, 2)].coverage == 100.0 and [(s.rate, s.offset, s.short_first, s.short_last, s.first, s.last, s.aligned)
                                             for s in by[(1, 2)].segments] == [
        (1, 50, 0, 39, 50, 89, 40), (-1, 479, 40, 79, 400, 439, 40), (-2, 460, 80, 109, 242, 300, 30)]
    default = search.signed_excerpt_pairs(blobs, matcher=SG.ReferenceMatcher)  # ((1, 1), (-1, 1)): the reel's 2x piece is left out
    assert [(e.short, e.long, int(e.coverage)) for e in default] == [(0, 2, 100), (1, 2, 72)]
    forward = search.rate_segmented_excerpt_pairs(blobs, matcher=SG.ReferenceMatcher)
    assert forward == []
    positive = ((1, 1), (2, 1), (3, 2))
    vids2 = RH.mixed_library(75) + list(RS.reel_c())
    blobs2 = [v.tobytes() for v in vids2]
    assert search.signed_excerpt_pairs(blobs2, rates=positive, matcher=SG.ReferenceMatcher) == \
        search.rate_segmented_excerpt_pairs(blobs2, rates=positive, matcher=SG.ReferenceMatcher) != []


# ---- the source shape and the code shape of the new kernel ----

def test_the_new_file_has_the_shape_of_its_siblings():
    src = "k_valign_signed.hip"
    text = open(os.path.join(CSRC, src)).read()
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    assert len(re.findall(r"\blaunch_lds_then_scratch\(op,", text)) == 1
    assert re.findall(r"hipLaunchKernelGGL\((\w+)<decltype\(big\)::value>, dim3\((\w+)\), dim3\(256\)", text) == [(src[:-4], "grid")]
    assert text.count("hipLaunchKernelGGL") == 1 and '#include "hvd_valign_dev.h"' in text
    assert "asm" not in text
    assert "hvd::signed_rate_list_length(nums, dens, revs)" in text
    kernels_h = open(os.path.join(CSRC, "hvd_kernels.h")).read()
    assert "constexpr uint32_t signed_rate_list_length(uint32_t nums, uint32_t dens, uint32_t revs)" in kernels_h
    assert "inline bool pack_signed_rate_list(" in kernels_h
    assert "launch_valign_rate_segments, launch_valign_signed};" in open(os.path.join(CSRC, "k_valign.hip")).read()
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert make.count("k_valign_signed.o") == 3  # OBJS, the asan link line, the hvd_valign_dev.h dependency line
    assert re.search(r"^k_valign_signed\.o: hvd_valign_dev\.h$", make, re.M)  # (a line of its own: the siblings' line is pinned)
    assert " k_valign_signed " in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    return _compile("k_valign_signed.hip", str(tmp_path_factory.mktemp("signed_shape")))


@pytest.mark.parametrize("name", ["k_valign_signed<false>", "k_valign_signed<true>"])
def test_signed_kernels_keep_their_budget(shapes, name):
    """DESIGN 4.25 budget, the siblings', read from the code-object metadata: no spilled register, no scratch, 256-lane
    workgroups; the LDS form within 32 768 B, so that five workgroups share a CU's LDS, and within the VGPRs of five waves
    per SIMD. The LDS form's histogram is a __shared__ array, so its votes are LDS atomics; the scratch form holds none."""
    assert sorted(shapes) == ["k_valign_signed<false>", "k_valign_signed<true>"]
    k = shapes[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0
    assert k["wg"] == 256
    if name == "k_valign_signed<false>":
        assert 4 * 4096 < k["lds"] <= 32768 and 5 * k["lds"] <= LDS_PER_CU, k["lds"]  # (the histogram lies in LDS)
        assert waves_per_simd(k["vgpr"] + k["agpr"]) >= 5, k["vgpr"]
    else:
        assert k["lds"] < 4 * 4096  # no histogram in LDS
