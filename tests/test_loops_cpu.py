"""Looped clips and boomerangs without a GPU: the numpy restatement of the rule (tests/loops_helpers.py) gives the
figures of the table the feature was proposed on -- a boomerang, a five-fold and a twelve-fold loop of an excerpt, a threefold
boomerang, none of which the signed alignment covers by more than one repetition -- and has the consequences the header states;
list soundness; the host entry refuses a broken list, max_rounds 0 and 65 and min_band_votes 0 before it asks for a device; the
scratch size; the fold's orientation choice, tie rules and edges; the header, the dtype and the surfaces; the new kernel compiles
for gfx950 inside its siblings' budget."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import loops_helpers as LH
import rates_helpers as RH
import signed_helpers as SG
from conftest import ROOT
from test_code_shape import HIPCC, LDS_PER_CU, _compile, waves_per_simd

CSRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
HEAD = ("a", "b", "q_hits", "t_hits", "n_segments", "q_covered", "t_covered", "rounds")


def lines(rounds):
    """(rate, offset, q_aligned) of every round."""
    return [((s[8], s[9]), s[0], s[2]) for s in rounds]


# ---- the table ----

def test_boomerang_is_whole_in_two_rounds():
    t = LH.table()
    source, boom = t["source"], t["boom"]
    assert len(source) == 600 and len(boom) == 120
    today = SG.signed_pair(boom, source, min_band_votes=4)[2]
    assert lines(today) == [((1, 1), 100, 61)] and 100 * 61 // 120 == 50  # today: one segment, 61 of 120
    q_hits, t_hits, rounds, t_covered = LH.loops_pair(boom, source, min_band_votes=4)
    assert lines(rounds) == [((1, 1), 100, 61), ((-1, 1), 219, 59)]
    assert sum(s[2] for s in rounds) == 120 == q_hits and t_covered == 60 == t_hits
    assert sum(s[3] for s in rounds) > t_covered  # a frame of the source sits in both rounds


def test_five_fold_loop():
    t = LH.table()
    source, loop5 = t["source"], t["loop5"]
    assert len(loop5) == 300
    assert lines(SG.signed_pair(loop5, source, min_band_votes=4)[2]) == [((1, 1), -20, 60)]  # today: 60 of 300
    _, _, rounds, t_covered = LH.loops_pair(loop5, source, min_band_votes=4)
    assert lines(rounds) == [((1, 1), d, 60) for d in (-20, 40, -80, 100, -140)]
    assert sum(s[2] for s in rounds) == 300 and t_covered == 60


def test_twelve_fold_loop_needs_more_than_eight_rounds():
    t = LH.table()
    source, loop12 = t["source"], t["loop12"]
    assert len(loop12) == 240
    today = SG.signed_pair(loop12, source, min_band_votes=4)[2]
    assert len(today) == 1 and today[0][2] == 20  # today: 20 of 240
    _, _, eight, t_covered = LH.loops_pair(loop12, source, max_rounds=8, min_band_votes=4)
    assert len(eight) == 8 and sum(s[2] for s in eight) == 160 and t_covered == 20
    _, _, rounds, t_covered = LH.loops_pair(loop12, source, max_rounds=64, min_band_votes=4)
    assert len(rounds) == 12 and sum(s[2] for s in rounds) == 240 and t_covered == 20
    rec = LH.record(0, 1, 240, 20, rounds, t_covered)
    assert int(rec["rounds"]) == 12 and int(rec["n_segments"]) == 8 and int(rec["q_covered"]) == 240
    assert rec["seg"].tolist() == [tuple(s) for s in rounds[:8]]  # rounds nine and later write no segment


def test_threefold_boomerang():
    t = LH.table()
    source, boom3 = t["source"], t["boom3"]
    assert len(boom3) == 180
    today = SG.signed_pair(boom3, source, min_band_votes=4)[2]
    assert len(today) == 1 and today[0][2] == 32  # today: 32 of 180
    _, _, rounds, t_covered = LH.loops_pair(boom3, source, min_band_votes=4)
    assert len(rounds) == 6 and sorted(s[8] for s in rounds) == [-1, -1, -1, 1, 1, 1]
    assert sum(s[2] for s in rounds) == 180 and t_covered == 30


def test_static_pair_and_plain_excerpt_are_the_signed_segment():
    A, B = LH.static_pair()
    today = SG.signed_pair(A, B, min_band_votes=4)[2]
    assert today == [(1, 150, 50, 52, 0, 49, 0, 51, 1, 1, 0, 0)]
    q_hits, t_hits, rounds, t_covered = LH.loops_pair(A, B, min_band_votes=4)
    assert rounds == today and t_covered == 52  # every frame of a is taken: the pair stops
    t = LH.table()
    today = SG.signed_pair(t["clip"], t["source"], min_band_votes=4)
    got = LH.loops_pair(t["clip"], t["source"], min_band_votes=4)
    assert len(today[2]) == 1 and today[2][0][2] == 60 and got[:3] == today and got[3] == 60


# ---- the consequences ----

@pytest.fixture(scope="module")
def planted():
    vids, pairs = LH.planted_loops(83)
    frames, offsets = RH.join(vids)
    t = LH.table()
    tf, to = RH.join([t["source"], t["boom"], t["loop5"], t["loop12"], t["boom3"], t["clip"]])
    return [(frames, offsets, pairs), (tf, to, [(v, 0) for v in range(1, 6)] + [(0, v) for v in range(1, 6)])]


def test_1_first_segment_and_hit_counts_are_the_signed_entrys(planted):
    for frames, offsets, pairs in planted:
        for rates, floor in ((LH.REVERSED_RATES, 1), (LH.REVERSED_RATES, 4), (SG.FOUR_RATES, 1), (((-1, 1), (1, 1)), 2)):
            got = LH.align_loops(frames, offsets, pairs, rates=rates, min_band_votes=floor)
            want = SG.align_signed(frames, offsets, pairs, rates=rates, min_band_votes=floor)
            assert np.array_equal(got["q_hits"], want["q_hits"]) and np.array_equal(got["t_hits"], want["t_hits"])
            assert np.array_equal(got["seg"][:, 0], want["seg"][:, 0])
            assert (got["n_segments"] >= 1).any()


def test_2_band_votes_never_increase(planted):
    checked = 0
    for frames, offsets, pairs in planted:
        for k, (a, b) in enumerate(pairs):
            got = LH.loops_pair(frames[offsets[a]:offsets[a + 1]], frames[offsets[b]:offsets[b + 1]], rates=SG.FOUR_RATES)
            votes = [s[1] for s in got[2]]
            assert votes == sorted(votes, reverse=True)
            checked += len(votes) >= 2
    assert checked >= 8


def test_3_q_covered_is_the_sum_over_the_stored_segments(planted):
    for frames, offsets, pairs in planted:
        got = LH.align_loops(frames, offsets, pairs, min_band_votes=2)
        few = got["rounds"] <= 8
        assert few.any() and (~few).any()
        assert np.array_equal(got["q_covered"][few], got["seg"]["q_aligned"][few].sum(1))
        assert (got["q_covered"][~few] > got["seg"]["q_aligned"][~few].sum(1)).all()
        assert (got["t_covered"] <= got["t_hits"]).all() and np.array_equal(got["n_segments"], np.minimum(got["rounds"], 8))


def test_4_one_round_is_the_signed_record_at_one_segment(planted):
    for frames, offsets, pairs in planted:
        got = LH.align_loops(frames, offsets, pairs, max_rounds=1, min_band_votes=3)
        want = SG.align_signed(frames, offsets, pairs, max_segments=1, min_band_votes=3)
        assert (got["rounds"] == got["n_segments"]).all() and set(got["rounds"].tolist()) <= {0, 1} and (got["rounds"] == 1).any()
        g, w = got.copy(), want.copy().view(LH.VLOOPS_DTYPE)
        g["rounds"] = 0
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        # and a pair that a full run ends after one round
        full = LH.align_loops(frames, offsets, pairs, min_band_votes=3)
        one = full["rounds"] == 1
        assert one.any() and np.array_equal(full[one], got[one])


# ---- list soundness ----

def test_list_soundness():
    rng = np.random.default_rng(84)
    frames, offsets = RH.join([RH._rand(rng, 5), RH._rand(rng, 7)])
    assert len(SG.BROKEN_LISTS) == 7
    for bad in SG.BROKEN_LISTS:
        assert LH.align_loops(frames, offsets, [(0, 1)], rates=bad)[0] == LH.lost_record(0, 1)
    assert LH.align_loops(frames, offsets, [(0, 1)], rates=SG.WIDE_SIGNED)[0] != LH.lost_record(0, 1)


def test_host_entry_refuses_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()  # (no hvd_init here: a sound call's answer depends on the library's state, none is made)
    rng = np.random.default_rng(85)
    frames, offsets = RH.join([RH._rand(rng, 5), RH._rand(rng, 7)])
    out = np.zeros(1, dtype=LH.VLOOPS_DTYPE)

    def call(rates, n_rates=None, max_rounds=64, min_band_votes=1, pair=(0, 1), positions=None):
        r = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
        pairs = np.array([pair], dtype=np.uint32)
        pos = None if positions is None else positions.ctypes.data
        return lib.hvd_vpdq_align_loops(frames.ctypes.data, offsets.ctypes.data, 2, pos, frames.ctypes.data, offsets.ctypes.data, 2, pos,
                                        pairs.ctypes.data, 1, 31, 1, r.ctypes.data if r.size else None,
                                        len(r) if n_rates is None else n_rates, max_rounds, min_band_votes, out.ctypes.data)

    for bad in SG.BROKEN_LISTS:
        assert call(bad) == _lib.HVD_ERR_ARG, bad
        assert "rates" in _lib.last_error()
    assert call(LH.REVERSED_RATES, n_rates=0) == _lib.HVD_ERR_ARG and call(LH.REVERSED_RATES, n_rates=9) == _lib.HVD_ERR_ARG
    for k in (0, 65, -1):
        assert call(LH.REVERSED_RATES, max_rounds=k) == _lib.HVD_ERR_ARG and "max_rounds" in _lib.last_error()
    assert call(LH.REVERSED_RATES, min_band_votes=0) == _lib.HVD_ERR_ARG and "min_band_votes" in _lib.last_error()
    assert call(LH.REVERSED_RATES, pair=(0, 2)) == _lib.HVD_ERR_ARG and "outside" in _lib.last_error()
    positions = np.concatenate([np.arange(5), np.arange(6), [131071]]).astype(np.int32)
    assert call([(1, 1), (-1, 8)], positions=positions) == _lib.HVD_ERR_ARG and "2^20" in _lib.last_error()
    assert not out.view(np.uint32).any()
    # the signed entry keeps its limit of eight
    out8 = np.zeros(1, dtype=SG.VSSEGMENTS_DTYPE)
    r = np.asarray(LH.REVERSED_RATES, dtype=np.int32)
    pairs = np.array([(0, 1)], dtype=np.uint32)
    assert lib.hvd_vpdq_align_signed(frames.ctypes.data, offsets.ctypes.data, 2, None, frames.ctypes.data, offsets.ctypes.data, 2, None,
                                     pairs.ctypes.data, 1, 31, 1, r.ctypes.data, 2, 9, 1, out8.ctypes.data) == _lib.HVD_ERR_ARG
    assert "max_segments" in _lib.last_error()


def test_scratch_size_follows_three_runs(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    sb, sb2 = C.c_size_t(1), C.c_size_t(2)
    for bins in (0, 1, 4096):
        assert lib.hvd_loops_scratch_bytes(bins, C.byref(sb)) == _lib.HVD_OK and sb.value == 0
    assert lib.hvd_loops_scratch_bytes(7202, C.byref(sb)) == _lib.HVD_OK and sb.value == 64 * 4 * (7202 + 3 * (7203 // 32 + 3))
    assert lib.hvd_signed_scratch_bytes(7202, C.byref(sb2)) == _lib.HVD_OK and sb2.value == 64 * 4 * (7202 + 2 * (7203 // 32 + 3))
    assert lib.hvd_loops_scratch_bytes(1 << 20, C.byref(sb)) == _lib.HVD_OK and sb.value == 64 * 4 * ((1 << 20) + 3 * (32768 + 3))
    assert lib.hvd_loops_scratch_bytes((1 << 20) + 1, C.byref(sb)) == _lib.HVD_ERR_ARG
    assert lib.hvd_loops_scratch_bytes(-1, C.byref(sb)) == _lib.HVD_ERR_ARG


# ---- the fold ----

def made(a, b, q_covered, t_covered, rounds, first=None):
    """A record with `rounds` rounds, the first of them (offset, q_aligned, t_aligned, (q_first, q_last), (t_first, t_last),
    (num, den), index) or a forward line at 0."""
    rec = np.zeros((), dtype=LH.VLOOPS_DTYPE)
    rec["a"], rec["b"], rec["q_covered"], rec["t_covered"], rec["rounds"] = a, b, q_covered, t_covered, rounds
    rec["q_hits"], rec["t_hits"], rec["n_segments"] = q_covered, t_covered, min(rounds, 8)
    d, qa, ta, qs, ts, rate, index = first or (0, q_covered, t_covered, (0, q_covered - 1), (0, t_covered - 1), (1, 1), 0)
    for k in range(min(rounds, 8)):
        rec["seg"][k] = (d, max(qa, ta), qa, ta) + qs + ts + rate + (index, 0)
    return rec


def test_fold_chooses_the_orientation_on_the_five_fold_loop(hvd):
    from fractions import Fraction

    from hvd_amd import search

    t = LH.table()
    frames, offsets = RH.join([t["source"], t["loop5"]])
    for pairs in ([(0, 1), (1, 0)], [(1, 0), (0, 1)]):  # the source against the loop, in both orders of the list
        recs = LH.align_loops(frames, offsets, pairs, min_band_votes=4)
        by = {(int(r["a"]), int(r["b"])): r for r in recs}
        assert int(by[0, 1]["q_covered"]) == 60 and int(by[0, 1]["rounds"]) == 1  # the source as a: 60 of 600, one round
        assert int(by[1, 0]["q_covered"]) == 300 and int(by[1, 0]["rounds"]) == 5
        (e,) = search.looped_excerpts_from_records(recs, [600, 300], np.array([7.0, 7.0]))
        assert (e.loop, e.source, e.coverage, e.similarity, e.rounds, e.source_frames) == (1, 0, 100.0, 7.0, 5, 60)
        assert [(s.rate, s.offset, s.short_first, s.short_last, s.first, s.last, s.aligned) for s in e.segments] == [
            (Fraction(1), Fraction(100 - 60 * k), 60 * k, 60 * k + 59, 100, 159, 60) for k in range(5)]
        assert all(isinstance(s, search.RateSegment) for s in e.segments)


def test_fold_tie_rules_on_a_full_copy(hvd):
    from hvd_amd import search

    lengths = [40, 40, 40]
    # the same percentage both ways: fewer rounds wins, whichever comes first in the list
    recs = np.array([made(0, 1, 40, 40, 2), made(1, 0, 40, 40, 1)], dtype=LH.VLOOPS_DTYPE)
    for order in ([0, 1], [1, 0]):
        (e,) = search.looped_excerpts_from_records(recs[order], lengths, np.ones(2))
        assert (e.loop, e.source, e.rounds) == (1, 0, 1)
    # the same percentage and the same rounds: the lower video index is a
    recs = np.array([made(2, 1, 40, 40, 1), made(1, 2, 40, 40, 1)], dtype=LH.VLOOPS_DTYPE)
    for order in ([0, 1], [1, 0]):
        (e,) = search.looped_excerpts_from_records(recs[order], lengths, np.ones(2))
        assert (e.loop, e.source, e.rounds, e.coverage) == (1, 2, 1, 100.0)
    # the percentage comes first: 100 % in three rounds beats 97 % (39 of 40) in one round
    recs = np.array([made(0, 1, 39, 39, 1), made(1, 0, 40, 40, 3)], dtype=LH.VLOOPS_DTYPE)
    (e,) = search.looped_excerpts_from_records(recs, lengths, np.ones(2))
    assert (e.loop, e.source, e.rounds) == (1, 0, 3)
    # one orientation alone is read as it stands
    (e,) = search.looped_excerpts_from_records(recs[:1], lengths, np.ones(1))
    assert (e.loop, e.source, int(e.coverage)) == (0, 1, 97)


def test_fold_edges_lost_and_empty(hvd):
    from hvd_amd import search

    lengths = [200, 40, 0]
    at = lambda q: np.array([made(0, 1, q, 30, 3)], dtype=LH.VLOOPS_DTYPE)  # noqa: E731
    assert [int(e.coverage) for e in search.looped_excerpts_from_records(at(100), lengths, np.ones(1))] == [50]
    assert search.looped_excerpts_from_records(at(99), lengths, np.ones(1)) == []  # 49.5 %
    assert len(search.looped_excerpts_from_records(at(99), lengths, np.ones(1), threshold=49.9)) == 1  # int(threshold)
    assert search.looped_excerpts_from_records(np.array([made(0, 1, 0, 0, 0)], dtype=LH.VLOOPS_DTYPE), lengths, np.ones(1), 1.0) == []
    lost = np.array([LH.lost_record(0, 1), made(1, 2, 40, 0, 1), made(2, 1, 0, 0, 0)], dtype=LH.VLOOPS_DTYPE)
    assert search.looped_excerpts_from_records(lost, lengths, np.ones(3)) == []
    with pytest.raises(ValueError):
        search.looped_excerpts_from_records(at(100), lengths, np.ones(1), threshold=0.5)


def test_search_on_the_reference_matcher(hvd):
    """A boomerang and a twelve-fold loop of an excerpt come back at coverage 100; the signed search reports neither at 100 and
    drops the loop; min_aligned is the alignment's floor."""
    from hvd_amd import search

    t = LH.table()
    rng = np.random.default_rng(86)
    vids = [t["boom"], t["loop12"], t["source"], t["clip"], RH._rand(rng, 30)]
    blobs = [v.tobytes() for v in vids]
    got = search.looped_excerpt_pairs(blobs, matcher=LH.ReferenceMatcher)
    by = {(e.loop, e.source): e for e in got}
    assert sorted(by) == [(0, 2), (1, 2), (3, 2)] and got == sorted(got)
    assert (by[0, 2].coverage, by[0, 2].rounds, by[0, 2].source_frames, len(by[0, 2].segments)) == (100.0, 2, 60, 2)
    assert sorted(s.rate for s in by[0, 2].segments) == [-1, 1]
    assert (by[1, 2].coverage, by[1, 2].rounds, by[1, 2].source_frames, len(by[1, 2].segments)) == (100.0, 12, 20, 8)
    assert (by[3, 2].coverage, by[3, 2].rounds, by[3, 2].source_frames) == (100.0, 1, 60)  # a plain excerpt: one round
    eight = {(e.loop, e.source): e for e in search.looped_excerpt_pairs(blobs, max_rounds=8, matcher=LH.ReferenceMatcher)}
    assert int(eight[1, 2].coverage) == 66 and eight[1, 2].rounds == 8
    today = {(e.short, e.long): int(e.coverage) for e in search.signed_excerpt_pairs(blobs, matcher=SG.ReferenceMatcher)}
    assert today == {(0, 2): 50, (3, 2): 100}
    # min_aligned: a round needs that many hits in its band -- 21 leaves the 20-frame repetitions of loop12 out
    high = {(e.loop, e.source) for e in search.looped_excerpt_pairs(blobs, min_aligned=21, matcher=LH.ReferenceMatcher)}
    assert high == {(0, 2), (3, 2)}
    assert {(e.loop, e.source) for e in search.looped_excerpt_pairs(blobs, min_aligned=20, matcher=LH.ReferenceMatcher)} == set(by)


# ---- surface shape ----

def test_header_dtype_and_surfaces(hvd):
    from hvd_amd import _lib, pipeline, search

    assert _lib.VLOOPS_DTYPE == LH.VLOOPS_DTYPE and _lib.VLOOPS_DTYPE.itemsize == 416 and _lib.ALIGN_MAX_ROUNDS == 64
    assert _lib.VLOOPS_DTYPE.names[:8] == HEAD and _lib.VLOOPS_DTYPE.fields["seg"][1] == 32
    assert _lib.VLOOPS_DTYPE.fields["rounds"][1] == _lib.VSSEGMENTS_DTYPE.fields["reserved"][1] == 28
    hdr = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert "#define HVD_ABI_VERSION 6 " in hdr and "#define HVD_ALIGN_MAX_ROUNDS 64" in hdr
    body = re.search(r"typedef struct hvd_vloops \{(.*?)\} hvd_vloops;", hdr, re.S).group(1)
    names = tuple(n.strip() for d in body.split(";") if d.strip() for n in d.split(None, 1)[1].split(","))
    assert names == HEAD + ("seg[HVD_ALIGN_MAX_SEGMENTS]",) and "hvd_vssegment seg" in body
    abi = re.search(r"#define HVD_ABI_VERSION 6 /\*(.*?)\*/", hdr).group(1)
    for name, twin in (("hvd_vpdq_align_loops", "hvd_vpdq_align_signed"), ("hvd_dev_vpdq_align_loops", "hvd_dev_vpdq_align_signed"),
                       ("hvd_loops_scratch_bytes", "hvd_signed_scratch_bytes")):
        assert re.search(rf"\bint {name}\(", hdr) and name in abi
        n_args = len(re.search(rf"\bint {name}\((.*?)\);", hdr, re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]) and _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    assert sorted(search.ALIGN_ROWS) == [(False, False), (False, True), (True, False), (True, True)]
    mode = search.AlignMode(search.REVERSED_RATES, 64, 4, loops=True)
    assert mode.loops is True and mode.signed is True and search.AlignMode().loops is False
    assert mode.row is search.LOOPS_ROW and search.AlignMode(search.REVERSED_RATES, 8, 1, True).row is search.SIGNED_ROW
    assert mode._replace(min_band_votes=2).row is search.LOOPS_ROW and isinstance(mode, search.AlignMode)
    assert tuple(mode) == (search.REVERSED_RATES, 64, 4, True)
    row = search.LOOPS_ROW
    assert row not in search.ALIGN_ROWS.values() and row is not search.SIGNED_ROW
    assert row.dtype == _lib.VLOOPS_DTYPE and row.method == "align_loops" and callable(getattr(search, row.method))
    assert (row.host_entry, row.device_entry, row.scratch_entry) == ("hvd_vpdq_align_loops", "hvd_dev_vpdq_align_loops",
                                                                      "hvd_loops_scratch_bytes")
    assert (row.excerpt, row.segment) == (search.LoopedExcerpt, search.RateSegment)
    assert search.LoopedExcerpt._fields == ("loop", "source", "coverage", "similarity", "rounds", "source_frames", "segments")
    assert hvd.find_looped_excerpts is search.find_looped_excerpts
    assert callable(search.looped_excerpts_from_records) and callable(search.looped_excerpt_pairs)
    assert callable(pipeline.find_looped_excerpts_on_device) and callable(pipeline.DeviceLibrary.align_loops)
    assert callable(hvd.Vpdq.align_loops) and hvd.DeviceLibrary is pipeline.DeviceLibrary


def test_the_new_file_has_the_shape_of_its_siblings():
    src = "k_valign_loops.hip"
    text = open(os.path.join(CSRC, src)).read()
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    assert len(re.findall(r"\blaunch_lds_then_scratch\(op,", text)) == 1
    assert re.findall(r"hipLaunchKernelGGL\((\w+)<decltype\(big\)::value>, dim3\((\w+)\), dim3\(256\)", text) == [(src[:-4], "grid")]
    assert text.count("hipLaunchKernelGGL") == 1 and '#include "hvd_valign_dev.h"' in text
    assert "asm" not in text
    assert "hvd::signed_rate_list_length(nums, dens, revs)" in text
    assert len(re.findall(r"scan_pair<[12], true, true>\(", text)) == 2  # scan_pair as it is: b's taken words stay zero
    assert "launch_valign_loops(mode, op, s)" in open(os.path.join(CSRC, "k_valign.hip")).read()
    kernels_h = open(os.path.join(CSRC, "hvd_kernels.h")).read()
    assert "static AlignMode of_loops(int max_rounds, int min_band_votes)" in kernels_h and "loops ? 5u" in kernels_h
    assert "unsigned slot_runs() const { return loops ? 3u : runs(); }" in kernels_h
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert make.count("k_valign_loops.o") == 3  # OBJS, the asan link line, the hvd_valign_dev.h dependency line
    assert re.search(r"^k_valign_loops\.o: hvd_valign_dev\.h$", make, re.M)
    assert " k_valign_loops " in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    return _compile("k_valign_loops.hip", str(tmp_path_factory.mktemp("loops_shape")))


@pytest.mark.parametrize("name", ["k_valign_loops<false>", "k_valign_loops<true>"])
def test_loops_kernels_keep_their_budget(shapes, name):
    """DESIGN 4.26 budget, read from the code-object metadata: no spilled register, no scratch, 256-lane workgroups; the LDS
    form holds the histogram and three pairs of runs of bit words and still lets five workgroups share a CU's LDS, within the
    VGPRs of five waves per SIMD; the scratch form holds no histogram in LDS."""
    assert sorted(shapes) == ["k_valign_loops<false>", "k_valign_loops<true>"]
    k = shapes[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0
    assert k["wg"] == 256
    if name == "k_valign_loops<false>":
        assert 4 * (4096 + 3 * 132) < k["lds"] <= 32768 and 5 * k["lds"] <= LDS_PER_CU, k["lds"]
        assert waves_per_simd(k["vgpr"] + k["agpr"]) >= 5, k["vgpr"]
    else:
        assert k["lds"] < 4 * 4096  # no histogram in LDS
