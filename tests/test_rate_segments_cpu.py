"""Rate-aware multi-segment alignment without a GPU: the numpy restatement of the rule
(tests/rate_segments_helpers.py) has the four consequences the header states, and gives the records of the two reels the feature
was proposed on -- which neither the slope-one peel nor the one-line rate search reports; the keep rule on hand-made records; the
header, the dtypes and the signatures; the host entry refuses broken calls before it touches the device; the new kernel file has
the shape of its three siblings and compiles for gfx950 inside their budget."""
import ctypes as C
import os
import re
import shutil
from fractions import Fraction

import numpy as np
import pytest

import rate_segments_helpers as RS
import rates_helpers as RH
import segments_helpers as SH
from conftest import ROOT
from test_code_shape import HIPCC, LDS_PER_CU, _compile, waves_per_simd

CSRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
HEAD = ("a", "b", "q_hits", "t_hits", "n_segments", "q_covered", "t_covered", "reserved")


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def check_identities(frames, offsets, pairs, positions=None, slack=1, max_dist=31, rates=RH.DEFAULT_RATES):
    """(a), (b), (c), (d) of the header on the restatement, against the restatements of the two sibling rules."""
    full = RS.align_rate_segments(frames, offsets, pairs, positions, rates, slack, max_dist)
    # (a) the list [(1, 1)]: the head and words 0-7 of every segment are the slope-one peel's, words 8-11 of a used one 1, 1, 0, 0
    for floor in (1, 4):
        unit = RS.align_rate_segments(frames, offsets, pairs, positions, ((1, 1),), slack, max_dist, min_band_votes=floor)
        peel = SH.align_segments(frames, offsets, pairs, positions, max_dist, slack, min_band_votes=floor)
        for u, s in zip(unit, peel):
            assert [u[n] for n in HEAD] == [s[n] for n in HEAD]
            for k in range(RS.MAX_SEGMENTS):
                assert u["seg"][k].tolist()[:8] == s["seg"][k].tolist()
                assert u["seg"][k].tolist()[8:] == ((1, 1, 0, 0) if k < s["n_segments"] else (0, 0, 0, 0))
    # (b) one segment, no floor: the one-line rate search
    one = RS.align_rate_segments(frames, offsets, pairs, positions, rates, slack, max_dist, max_segments=1)
    line = RH.align_rates(frames, offsets, pairs, positions, rates, slack, max_dist)
    for o, r in zip(one, line):
        assert o.tolist()[:4] == r.tolist()[:4] and o["seg"][0].tolist() == r.tolist()[4:]
        assert o["n_segments"] == (1 if r["q_hits"] else 0) and not o["seg"][1:].view(np.uint32).any()
    three = RS.align_rate_segments(frames, offsets, pairs, positions, rates[:3], slack, max_dist, max_segments=3, min_band_votes=2)
    for f, o, t in zip(full, one, three):
        # (c) the counters depend on neither the list nor K
        assert (f["q_hits"], f["t_hits"]) == (o["q_hits"], o["t_hits"]) == (t["q_hits"], t["t_hits"])
        for rec in (f, t):
            segs = rec["seg"][:rec["n_segments"]]
            # (d) band_votes never increases; a segment's aligned frames never outnumber its band_votes
            assert (np.diff(segs["band_votes"].astype(np.int64)) <= 0).all()
            assert (segs["q_aligned"] <= segs["band_votes"]).all() and (segs["t_aligned"] <= segs["band_votes"]).all()
            assert rec["q_covered"] == segs["q_aligned"].sum() and rec["t_covered"] == segs["t_aligned"].sum()
        # the first segment does not depend on K
        assert f["seg"][0] == o["seg"][0]
    return full


@pytest.mark.parametrize("seed,slack", [(71, 1), (72, 0)])
def test_identities_on_planted_pieces(seed, slack):
    vids = SH.planted_pieces_library(seed, 31, lengths=(0, 1, 2, 3, 17, 64, 65, 130))
    frames, offsets = RH.join(vids)
    V = len(vids)
    pairs = [(v - 1, v) for v in range(1, V)] + [(v, v - 1) for v in range(1, V)]
    positions = None if slack else SH.gapped(np.random.default_rng(seed), offsets)
    full = check_identities(frames, offsets, pairs, positions, slack)
    assert (full["n_segments"] >= 2).sum() >= 4


def test_identities_on_every_pair_of_the_mixed_library():
    frames, offsets = RH.join(RH.mixed_library(73))
    V = len(offsets) - 1
    full = check_identities(frames, offsets, [(a, b) for a in range(V) for b in range(V)])
    assert (full["seg"][:, 0]["rate_index"] > 0).sum() >= 8  # the planted rates are found, in both orientations


def seg_words(segs):
    """(rate, offset, q_aligned) of every segment."""
    return [((s[8], s[9]), s[0], s[2]) for s in segs]


def test_reel_c_three_pieces_at_two_to_one():
    source, reel = RS.reel_c()
    assert len(source) == 600 and len(reel) == 90
    # neither sibling reports the pair: every band of slope one holds three frames, one line holds one piece of three
    assert SH.segments_of_pair(reel, source, min_band_votes=4) == (90, 90, [])
    line = RH.rates_pair(reel, source)
    assert line[4] == 30 and 100 * line[4] // 90 < 50
    q_hits, t_hits, segs = RS.rate_segments_pair(reel, source, min_band_votes=4)
    assert (q_hits, t_hits) == (90, 90)
    assert seg_words(segs) == [((2, 1), -9, 30), ((2, 1), 60, 30), ((2, 1), 300, 30)]
    assert [s[1:4] for s in segs] == [(30, 30, 30)] * 3 and [s[10] for s in segs] == [7, 7, 7]
    assert [(s[4], s[5]) for s in segs] == [(30, 59), (60, 89), (0, 29)]
    frames, offsets = RH.join([reel, source])
    check_identities(frames, offsets, [(0, 1), (1, 0)])


def test_reel_b_four_pieces_at_four_rates():
    source, reel = RS.reel_b()
    assert len(reel) == 150
    q_hits, t_hits, segs = RS.rate_segments_pair(reel, source, min_band_votes=4)
    assert seg_words(segs) == [((5, 4), 1149, 60), ((3, 2), 600, 40), ((2, 1), -29, 30), ((1, 1), 430, 20)]
    assert sum(s[2] for s in segs) == 150 == sum(s[3] for s in segs) and (q_hits, t_hits) == (150, 150)
    assert [s[10] for s in segs] == [RH.DEFAULT_RATES.index(s[8:10]) for s in segs]
    assert RS.rate_segments_pair(reel, source)[2] == segs  # the floor ends nothing here
    # one line covers 40 %; the slope-one peel reports 111 frames as eight fragments
    assert RH.rates_pair(reel, source)[4] == 60
    peel = SH.segments_of_pair(reel, source, min_band_votes=4)[2]
    assert len(peel) == 8 and sum(s[2] for s in peel) == 111
    # from the b side the default list has no (1, 2): the 2/1 piece goes to neighbouring rates in fragments
    back = RS.rate_segments_pair(source, reel, min_band_votes=4)[2]
    assert len(back) > 4 and sum(s[3] for s in back) >= 140
    whole = RS.rate_segments_pair(source, reel, rates=RH.list_with((1, 2)), min_band_votes=4)[2]
    assert ((1, 2), 29, 30) in [((s[8], s[9]), s[0], s[3]) for s in whole]
    frames, offsets = RH.join([reel, source])
    check_identities(frames, offsets, [(0, 1), (1, 0)])


def test_a_rate_that_needs_too_many_bins_loses_the_pair():
    rng = np.random.default_rng(74)
    A = rand(rng, 2)
    positions = np.array([0, 100000, 0, 248560], dtype=np.int32)
    frames, offsets = RH.join([A, A[::-1].copy()])
    got = RS.align_rate_segments(frames, offsets, [(0, 1), (0, 2)], positions, ((1, 1), (8, 1)))
    assert got[0] == RS.lost_record(0, 1) and got[1] == RS.lost_record(0, 2)
    assert RS.align_rate_segments(frames, offsets, [(0, 1)], positions, ((1, 1),))[0]["n_segments"] == 2
    assert RS.align_rate_segments(frames, offsets, [(0, 1)], None, ((2, 4),))[0] == RS.lost_record(0, 1)


# ---- header, dtypes, keep rule ----

def test_header_and_dtypes(hvd):
    from hvd_amd import _lib, pipeline, search

    assert _lib.VRSEGMENT_DTYPE == RS.VRSEGMENT_DTYPE and _lib.VRSEGMENT_DTYPE.itemsize == 48
    assert _lib.VRSEGMENTS_DTYPE == RS.VRSEGMENTS_DTYPE and _lib.VRSEGMENTS_DTYPE.itemsize == 416
    assert _lib.VRSEGMENT_DTYPE.names[:8] == _lib.VSEGMENT_DTYPE.names and _lib.VRSEGMENT_DTYPE.names[8:] == _lib.VRATE_DTYPE.names[12:]
    assert _lib.VRSEGMENTS_DTYPE.names[:8] == _lib.VSEGMENTS_DTYPE.names[:8] == HEAD
    assert _lib.VRSEGMENTS_DTYPE.fields["seg"][1] == 32 and _lib.VRSEGMENTS_DTYPE["seg"].shape == (_lib.ALIGN_MAX_SEGMENTS,)
    hdr = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert "#define HVD_ABI_VERSION 6 " in hdr
    for struct, dtype in (("hvd_vrsegment", _lib.VRSEGMENT_DTYPE), ("hvd_vrsegments", _lib.VRSEGMENTS_DTYPE)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, re.S).group(1)
        decls = [d.split(None, 1)[1] for d in body.split(";") if d.strip()]
        names = tuple(n.strip() for d in decls for n in d.split(","))
        assert names == dtype.names[:-1] + ("seg[HVD_ALIGN_MAX_SEGMENTS]",) if struct.endswith("s") else names == dtype.names
    abi = re.search(r"#define HVD_ABI_VERSION 6 /\*(.*?)\*/", hdr).group(1)
    for name in ("hvd_vpdq_align_rate_segments", "hvd_dev_vpdq_align_rate_segments", "hvd_rate_segments_scratch_bytes"):
        assert re.search(rf"\bint {name}\(", hdr) and name in _lib.SIGNATURES and name in abi
        n_args = len(re.search(rf"\bint {name}\((.*?)\);", hdr, re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert hvd.find_rate_segmented_excerpts is search.find_rate_segmented_excerpts
    assert callable(pipeline.find_rate_segmented_excerpts_on_device) and callable(pipeline.DeviceLibrary.align_rate_segments)
    assert callable(hvd.Vpdq.align_rate_segments)
    assert search.RateSegment._fields == ("rate", "offset", "short_first", "short_last", "first", "last", "aligned")
    assert search.RateSegmentedExcerpt._fields == ("short", "long", "coverage", "similarity", "segments")


def made_record(a, b, segs):
    """segs: (offset, q_aligned, t_aligned, (q_first, q_last), (t_first, t_last), (num, den), index)."""
    full = [(d, max(qa, ta), qa, ta) + qs + ts + rate + (index, 0) for d, qa, ta, qs, ts, rate, index in segs]
    return RS.record(a, b, sum(s[2] for s in full), sum(s[3] for s in full), full)


def test_keep_rule_orientation_floor_and_threshold_edge(hvd):
    from hvd_amd import search

    RSeg, RSE = search.RateSegment, search.RateSegmentedExcerpt
    lengths = [40, 100, 40, 8, 0]
    recs = np.array([
        # a is short: p_b = 5/4 p_a + 81/4 and p_b = 2 p_a - 9; a third segment of three frames is below min_aligned
        made_record(0, 1, [(81, 16, 17, (20, 38), (45, 67), (5, 4), 1), (-9, 12, 12, (2, 13), (0, 17), (2, 1), 7),
                           (7, 3, 3, (15, 17), (22, 24), (1, 1), 0)]),
        # b is short: p_a = 3/2 p_b + 45 and p_a = p_b + 4
        made_record(1, 2, [(-90, 30, 20, (45, 75), (0, 20), (2, 3), 6), (-4, 10, 10, (34, 43), (30, 39), (1, 1), 0)]),
        # equal lengths: a is short; 19 of 40 is 47.5 %
        made_record(0, 2, [(3, 10, 10, (0, 9), (3, 12), (1, 1), 0), (40, 9, 9, (20, 28), (40, 48), (2, 1), 7)]),
        made_record(3, 1, [(7, 3, 3, (0, 2), (7, 9), (1, 1), 0), (30, 3, 3, (4, 6), (34, 36), (1, 1), 0)]),  # below min_aligned
        RS.lost_record(1, 3),
        RS.record(4, 1, 0, 0, []),  # an empty video
        # equal lengths again: a = 2 is short, 12 + 8 of 40 is exactly 50 %
        made_record(2, 0, [(-4, 12, 12, (4, 18), (0, 11), (4, 5), 2), (10, 8, 9, (30, 37), (20, 28), (1, 2), 7)]),
    ], dtype=RS.VRSEGMENTS_DTYPE)
    sim = np.arange(7, dtype=np.float64)
    got = search.rate_segmented_excerpts_from_records(recs, lengths, sim)
    assert got == [
        RSE(0, 1, 70.0, 0.0, (RSeg(Fraction(2), Fraction(-9), 2, 13, 0, 17, 12), RSeg(Fraction(5, 4), Fraction(81, 4), 20, 38, 45, 67, 16))),
        RSE(2, 0, 50.0, 6.0, (RSeg(Fraction(4, 5), Fraction(-4, 5), 4, 18, 0, 11, 12), RSeg(Fraction(1, 2), Fraction(5), 30, 37, 20, 28, 8))),
        RSE(2, 1, 75.0, 1.0, (RSeg(Fraction(3, 2), Fraction(45), 0, 20, 45, 75, 20), RSeg(Fraction(1), Fraction(4), 30, 39, 34, 43, 10)))]
    assert all(isinstance(s.rate, Fraction) and isinstance(s.offset, Fraction) for e in got for s in e.segments)
    # the edge int(coverage) == int(threshold): 47.5 % passes 47.9 and fails 48
    assert (0, 2) in [(e.short, e.long) for e in search.rate_segmented_excerpts_from_records(recs, lengths, sim, threshold=47.9)]
    assert (0, 2) not in [(e.short, e.long) for e in search.rate_segmented_excerpts_from_records(recs, lengths, sim, threshold=48.0)]
    # the floor: at min_aligned = 3 the third segment of the first record counts and the three-frame pair is kept
    low = search.rate_segmented_excerpts_from_records(recs, lengths, sim, threshold=37.5, min_aligned=3)
    assert [(e.short, e.long, len(e.segments)) for e in low] == [(0, 1, 3), (0, 2, 2), (2, 0, 2), (2, 1, 2), (3, 1, 2)]
    assert low[0].coverage == 77.5 and low[4].coverage == 75.0
    assert search.rate_segmented_excerpts_from_records(recs, lengths, sim, min_aligned=21) == []
    # an INT32_MIN record is dropped whatever else it holds
    odd = recs.copy()
    odd[0]["seg"][0]["offset"] = RS.INT32_MIN
    assert (0, 1) not in [(e.short, e.long) for e in search.rate_segmented_excerpts_from_records(odd, lengths, sim)]
    with pytest.raises(ValueError):
        search.rate_segmented_excerpts_from_records(recs, lengths, sim, threshold=0.5)


def test_search_on_the_reference_matcher(hvd):
    """On the reference matchers: the unit list is the segmented search, one segment is the rate search, and reel C is reported
    by the new search alone."""
    from hvd_amd import search

    rng = np.random.default_rng(75)
    source, reel_c = RS.reel_c()
    vids = RH.mixed_library(75) + [reel_c, source, rand(rng, 30)]
    blobs = [v.tobytes() for v in vids]
    got = search.rate_segmented_excerpt_pairs(blobs, matcher=RS.ReferenceMatcher)
    by = {(e.short, e.long): e for e in got}
    c = by[(12, 13)]
    assert c.coverage == 100.0 and [(s.rate, s.offset, s.short_first, s.aligned) for s in c.segments] == [
        (2, 300, 0, 30), (2, -9, 30, 30), (2, 60, 60, 30)]
    assert (12, 13) not in {(e.short, e.long) for e in search.segmented_excerpt_pairs(blobs, matcher=RS.ReferenceMatcher)}
    assert (12, 13) not in {(e.short, e.long) for e in search.rate_excerpt_pairs(blobs, matcher=RS.ReferenceMatcher)}
    unit = search.rate_segmented_excerpt_pairs(blobs, rates=((1, 1),), matcher=RS.ReferenceMatcher)
    peel = search.segmented_excerpt_pairs(blobs, matcher=RS.ReferenceMatcher)
    assert len(peel) >= 2 and [e[:4] for e in unit] == [e[:4] for e in peel]
    assert [[tuple(s)[1:] for s in e.segments] for e in unit] == [[tuple(s) for s in e.segments] for e in peel]
    assert all(s.rate == 1 for e in unit for s in e.segments)
    one = search.rate_segmented_excerpt_pairs(blobs, max_segments=1, matcher=RS.ReferenceMatcher)
    line = search.rate_excerpt_pairs(blobs, matcher=RS.ReferenceMatcher)
    assert len(line) >= 4 and [(e.short, e.long, e.segments[0].rate, e.segments[0].offset, e.coverage) for e in one] == [
        (e.short, e.long, e.rate, e.offset, e.coverage) for e in line]


# ---- the host entry refuses a broken call before it touches the device ----

def test_host_entry_rejects_broken_calls_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()  # (no hvd_init: a sound call would be HVD_ERR_STATE here)
    rng = np.random.default_rng(76)
    frames, offsets = RH.join([rand(rng, 5), rand(rng, 7)])
    out = np.zeros(1, dtype=RS.VRSEGMENTS_DTYPE)

    def call(rates=((1, 1), (2, 1)), n_rates=None, max_segments=8, min_band_votes=1, pair=(0, 1), positions=None):
        r = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
        pairs = np.array([pair], dtype=np.uint32)
        pos = None if positions is None else positions.ctypes.data
        return lib.hvd_vpdq_align_rate_segments(frames.ctypes.data, offsets.ctypes.data, 2, pos, frames.ctypes.data,
                                                offsets.ctypes.data, 2, pos, pairs.ctypes.data, 1, 31, 1,
                                                r.ctypes.data if r.size else None, len(r) if n_rates is None else n_rates,
                                                max_segments, min_band_votes, out.ctypes.data)

    for bad in (RH.NINE_RATES, [(2, 4)], [(1, 1), (1, 1)], [(0, 1)], [(1, 9)]):  # test_gpu_rates.test_broken_lists'
        assert call(bad) == _lib.HVD_ERR_ARG, bad
        assert "rates" in _lib.last_error()
    assert call([]) == _lib.HVD_ERR_ARG and call(n_rates=0) == _lib.HVD_ERR_ARG and call(n_rates=9) == _lib.HVD_ERR_ARG
    for k in (0, 9, -1):
        assert call(max_segments=k) == _lib.HVD_ERR_ARG and "max_segments" in _lib.last_error()
    for floor in (0, -3):
        assert call(min_band_votes=floor) == _lib.HVD_ERR_ARG and "min_band_votes" in _lib.last_error()
    for pair in ((0, 2), (2, 0), (7, 7)):
        assert call(pair=pair) == _lib.HVD_ERR_ARG and "outside" in _lib.last_error()
    positions = np.concatenate([np.arange(5), np.arange(6), [131071]]).astype(np.int32)
    assert call([(1, 1), (1, 8)], positions=positions) == _lib.HVD_ERR_ARG and "2^20" in _lib.last_error()
    # (what a sound call gives depends on the library's state, not on its arguments: none is made here)
    assert not out.view(np.uint32).any()
    sb = C.c_size_t(1)
    assert lib.hvd_rate_segments_scratch_bytes(7202, C.byref(sb)) == _lib.HVD_OK and sb.value == 64 * 4 * (7202 + 2 * (225 + 3))
    assert lib.hvd_rate_segments_scratch_bytes(4096, C.byref(sb)) == _lib.HVD_OK and sb.value == 0
    assert lib.hvd_rate_segments_scratch_bytes((1 << 20) + 1, C.byref(sb)) == _lib.HVD_ERR_ARG


# ---- the source shape and the code shape of the new kernel ----

def test_the_new_file_has_the_shape_of_its_siblings():
    """What tests/test_align_many_pairs_shape.py asks of k_valign.hip, k_valign_segments.hip and k_valign_rates.hip."""
    src = "k_valign_rate_segments.hip"
    text = open(os.path.join(CSRC, src)).read()
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    assert len(re.findall(r"\blaunch_lds_then_scratch\(op,", text)) == 1
    assert re.findall(r"hipLaunchKernelGGL\((\w+)<decltype\(big\)::value>, dim3\((\w+)\), dim3\(256\)", text) == [(src[:-4], "grid")]
    assert text.count("hipLaunchKernelGGL") == 1 and '#include "hvd_valign_dev.h"' in text
    assert "asm" not in text
    # the taken words: two pairs of runs of bit words in a slot, read off the mode (hvd::alignment_scratch_bytes in k_valign.hip)
    assert "slot_scratch_bytes(max_bins, mode.runs())" in open(os.path.join(CSRC, "k_valign.hip")).read()
    assert "unsigned runs() const { return segmented ? 2u : 1u; }" in open(os.path.join(CSRC, "hvd_kernels.h")).read()
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert make.count("k_valign_rate_segments.o") == 3  # OBJS, the asan link line, the hvd_valign_dev.h dependency line
    assert re.search(r"^k_valign\.o .*k_valign_rate_segments\.o: hvd_valign_dev\.h$", make, re.M)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    return _compile("k_valign_rate_segments.hip", str(tmp_path_factory.mktemp("rate_segments_shape")))


@pytest.mark.parametrize("name", ["k_valign_rate_segments<false>", "k_valign_rate_segments<true>"])
def test_rate_segment_kernels_keep_their_budget(shapes, name):
    """DESIGN 4.18 budget, the siblings': no spilled register, no scratch, 256-lane workgroups; the LDS form stays within
    32 768 B, so that five workgroups share a CU's LDS, and within the VGPRs of five waves per SIMD, and votes with LDS atomics."""
    assert sorted(shapes) == ["k_valign_rate_segments<false>", "k_valign_rate_segments<true>"]
    k = shapes[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and "scratch_" not in k["isa"]
    assert k["wg"] == 256 and "v_bcnt_u32_b32" in k["isa"]
    if name == "k_valign_rate_segments<false>":
        assert k["lds"] <= 32768 and 5 * k["lds"] <= LDS_PER_CU, k["lds"]
        assert waves_per_simd(k["vgpr"] + k["agpr"]) >= 5, k["vgpr"]
        assert "ds_add_u32" in k["isa"] and "ds_or_b32" in k["isa"]
