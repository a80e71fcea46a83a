"""Highlight reels and re-cuts without a GPU: the numpy restatement of the multi-segment rule
(tests/segments_helpers.py) gives the hand-derived records and the rule's three consequences; the premise of the feature holds on
it -- the single-offset excerpt search drops a reel of five pieces, the segmented one reports it at coverage 100 and still
leaves the same frames in shuffled order alone; the new kernels compile for gfx950 within their budget."""
import os
import re
import shutil

import numpy as np
import pytest

import align_helpers as AH
import segments_helpers as SH
from conftest import ROOT
from test_code_shape import HIPCC, LDS_PER_CU, _compile, waves_per_simd


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


REEL_STARTS = (40, 410, 130, 520, 255)


def reel_library(seed=7):
    """L: 600 random frames. R: a reel of 5 x 12 frames of L from REEL_STARTS, up to 24 bits flipped. D: the frames of R in
    shuffled order."""
    rng = np.random.default_rng(seed)
    L = rand(rng, 600)
    R = AH.noisy(rng, np.concatenate([L[s:s + 12] for s in REEL_STARTS]), 24)
    D = R[np.random.default_rng(seed).permutation(60)]
    return [L, R, D]


# ---- the rule, on hand-derived cases ----

def test_reel_of_five_pieces():
    """Piece k (frames 12k .. 12k + 11 of the reel) sits at L[s_k ..]: offset s_k - 12k, 12 votes each. Equal S and equal votes
    leave the smaller |d|, so the segments come out in the order of their offsets: 40, 106, 207, 398, 484."""
    L, R, _ = reel_library()
    assert AH.align_pair(R, L)[2:6] == (40, 12, 12, 12)  # the single-offset rule sees one piece
    q_hits, t_hits, segs = SH.segments_of_pair(R, L)
    assert (q_hits, t_hits) == (60, 60)
    assert segs == [(40, 12, 12, 12, 0, 11, 40, 51), (106, 12, 12, 12, 24, 35, 130, 141), (207, 12, 12, 12, 48, 59, 255, 266),
                    (398, 12, 12, 12, 12, 23, 410, 421), (484, 12, 12, 12, 36, 47, 520, 531)]
    assert SH.segments_of_pair(R, L, max_segments=2)[2] == segs[:2]
    rec = SH.record(1, 0, q_hits, t_hits, segs)
    assert (rec["n_segments"], rec["q_covered"], rec["t_covered"]) == (5, 60, 60)
    assert rec["seg"][5:].tobytes() == bytes(3 * 32)  # unused slots are zero
    # the long video as a: the offsets change sign, the sides swap
    assert SH.segments_of_pair(L, R)[2][0] == (-40, 12, 12, 12, 40, 51, 0, 11)


def test_recut_with_a_dropped_frame():
    """L[100:115] + L[116:130] + L[300:330]: frames 0..14 at offset 100, 15..28 at 101, 29..58 at 271. Slack 1: votes[271] = 30
    wins round 1; round 2 has S(100) = S(101) = 29, votes 15 against 14: offset 100 absorbs the dropped frame L[115]."""
    rng = np.random.default_rng(21)
    L = rand(rng, 400)
    C = np.concatenate([L[100:115], L[116:130], L[300:330]])
    assert SH.segments_of_pair(C, L)[2] == [(271, 30, 30, 30, 29, 58, 300, 329), (100, 29, 29, 29, 0, 28, 100, 129)]
    # slack 0 splits the second segment at the dropped frame
    assert SH.segments_of_pair(C, L, slack=0)[2] == [(271, 30, 30, 30, 29, 58, 300, 329), (100, 15, 15, 15, 0, 14, 100, 114),
                                                     (101, 14, 14, 14, 15, 28, 116, 129)]


def test_static_videos_stop_after_one_segment():
    """50 frames against 80 of one image: the record of the single-offset rule (offset 1, band_votes 150, 50 and 52 aligned),
    and then every frame of a is taken."""
    h = rand(np.random.default_rng(1), 1)
    A, B = np.repeat(h, 50, axis=0), np.repeat(h, 80, axis=0)
    assert SH.segments_of_pair(A, B) == (50, 80, [(1, 150, 50, 52, 0, 49, 0, 51)])
    # the other way round 28 frames of the longer video are left, and nothing to match them with
    assert SH.segments_of_pair(B, A) == (80, 50, [(-1, 150, 52, 50, 0, 51, 0, 49)])


def test_two_diagonals_sharing_frames():
    """a's frames 4..13 sit at b 20..29 (offset 16, 10 votes), a's frames 0..7 at b 5..12 (offset 5, 8 votes). Round 1 takes
    a 4..13; round 2 is only what that left of the other diagonal: a 0..3 at b 5..8."""
    rng = np.random.default_rng(22)
    A, B = rand(rng, 14), rand(rng, 30)
    B[5:13] = A[0:8]
    B[20:30] = A[4:14]
    assert AH.align_pair(A, B)[:6] == (14, 18, 16, 10, 10, 10)
    assert SH.segments_of_pair(A, B) == (14, 18, [(16, 10, 10, 10, 4, 13, 20, 29), (5, 4, 4, 4, 0, 3, 5, 8)])
    # a frame of b shared by two diagonals: b 0..5 holds a 0..5, and a 8..11 holds b 2..5 again
    A, B = rand(rng, 12), rand(rng, 9)
    B[0:6] = A[0:6]
    A[8:12] = B[2:6]
    assert SH.segments_of_pair(A, B, slack=0) == (10, 6, [(0, 6, 6, 6, 0, 5, 0, 5)])  # round 2: b 2..5 are taken, H_2 is empty


def test_given_positions_with_gaps():
    """The hits of test_align_cpu's case: deltas 10, 10, 10, 13, 23. Slack 1: the band of 10 takes three frames, then the
    lone hits follow by |d|; a floor of two votes ends the pair after the first segment."""
    rng = np.random.default_rng(5)
    A, B = rand(rng, 5), rand(rng, 6)
    pa, pb = [0, 2, 3, 7, 8], [10, 12, 13, 20, 30, 31]
    B[0], B[1], B[2], B[3], B[5] = A[0], A[1], A[2], A[3], A[4]
    assert SH.segments_of_pair(A, B, pa, pb, slack=1) == (5, 5, [(10, 3, 3, 3, 0, 3, 10, 13), (13, 1, 1, 1, 7, 7, 20, 20),
                                                                 (23, 1, 1, 1, 8, 8, 31, 31)])
    assert SH.segments_of_pair(A, B, pa, pb, slack=1, min_band_votes=2)[2] == [(10, 3, 3, 3, 0, 3, 10, 13)]
    assert SH.segments_of_pair(A, B, pa, pb, slack=3)[2] == [(10, 4, 4, 4, 0, 7, 10, 20), (23, 1, 1, 1, 8, 8, 31, 31)]
    assert SH.segments_of_pair(A, B, pa, pb, slack=3, max_segments=1)[2] == [(10, 4, 4, 4, 0, 7, 10, 20)]


def test_no_hit_and_empty_videos_give_the_zero_record():
    rng = np.random.default_rng(4)
    A, B = rand(rng, 12), rand(rng, 9)
    assert AH.hamming_matrix(A, B).min() > 31
    assert SH.segments_of_pair(A, B) == (0, 0, []) and SH.segments_of_pair(A[:0], B) == (0, 0, [])
    recs = SH.align_segments(np.concatenate([A, B]), [0, 12, 12, 21], [(0, 2), (1, 2)])
    assert recs.tobytes() == np.array([0, 2] + [0] * 70 + [1, 2] + [0] * 70, dtype="<u4").tobytes()
    lost = SH.lost_record(3, 4)
    assert lost.tobytes() == np.array([3, 4] + [0] * 6 + [1 << 31] + [0] * 63, dtype="<u4").tobytes()


# ---- the three consequences of the rule, on randomized planted libraries ----

@pytest.mark.parametrize("seed", [31, 32, 33])
def test_consequences_on_planted_libraries(seed):
    rng = np.random.default_rng(seed)
    vids = SH.planted_pieces_library(seed, 31, lengths=(0, 3, 40, 64, 130, 90, 257))
    frames = np.concatenate(vids)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    pairs = [(a, b) for a in range(len(vids)) for b in range(len(vids))]
    positions = None if seed == 31 else SH.gapped(rng, offsets)
    slack = int(rng.integers(0, 3))
    single = AH.align_videos(frames, offsets, pairs, positions, 31, slack)
    multi = SH.align_segments(frames, offsets, pairs, positions, 31, slack)
    assert (multi["n_segments"] >= 2).sum() >= 4
    lengths = np.diff(offsets)
    for s, m in zip(single, multi):
        n = int(m["n_segments"])
        # (a) segment 1 is the single-offset record, word for word
        assert (m["a"], m["b"], m["q_hits"], m["t_hits"]) == (s["a"], s["b"], s["q_hits"], s["t_hits"])
        assert m["seg"][0].tolist() == tuple(s.tolist()[4:])
        # (b) band_votes never increases
        votes = m["seg"]["band_votes"][:n].astype(np.int64)
        assert (np.diff(votes) <= 0).all() and (votes >= 1).all()
        # (c) disjoint aligned sets: the covered counts are the sums, within the hits and the lengths
        assert m["q_covered"] == m["seg"]["q_aligned"][:n].sum() <= min(m["q_hits"], lengths[m["a"]])
        assert m["t_covered"] == m["seg"]["t_aligned"][:n].sum() <= min(m["t_hits"], lengths[m["b"]])
        assert m["seg"][n:].tobytes() == bytes(32 * (8 - n))
        # an aligned frame needs a vote in the band
        assert (m["seg"]["q_aligned"][:n] <= votes).all() and (m["seg"]["t_aligned"][:n] <= votes).all()
    # a smaller K gives a prefix, a floor cuts the tail
    for K, floor in ((1, 1), (2, 1), (8, 4)):
        cut = SH.align_segments(frames, offsets, pairs, positions, 31, slack, max_segments=K, min_band_votes=floor)
        for m, c in zip(multi, cut):
            n = min(K, int((m["seg"]["band_votes"][:int(m["n_segments"])] >= floor).sum()))
            assert c["n_segments"] == n and c["seg"][:n].tolist() == m["seg"][:n].tolist()


# ---- the premise: one offset drops the reel, the segments report it, the shuffle stays out ----

def test_premise_reel_is_found_and_the_shuffle_is_not(hvd):
    from hvd_amd import search

    L, R, D = reel_library()
    # the condition of the shuffled case, on the restatement: every segment is below min_aligned = 4
    _, _, shuffled = SH.segments_of_pair(D, L)
    assert shuffled and max(s[2] for s in shuffled) < 4, shuffled
    blobs = [L.tobytes(), R.tobytes(), D.tobytes()]
    # the single-offset search: 12 of 60 frames = 20 %, dropped at threshold 50 (and D with it)
    assert search.excerpt_pairs(blobs, 50.0, 4, 1, None, matcher=AH.ReferenceMatcher) == []
    assert [tuple(e[:3]) for e in search.excerpt_pairs(blobs, 20.0, 4, 1, None, matcher=AH.ReferenceMatcher)] == [(1, 0, 40)]
    got = search.segmented_excerpt_pairs(blobs, 50.0, 4, 1, None, matcher=SH.ReferenceMatcher)
    assert [(e.short, e.long, e.coverage) for e in got] == [(1, 0, 100.0)]
    assert int(got[0].similarity) == 10  # the counters: min(60 / 60, 60 / 600)
    assert got[0].segments == tuple(search.Segment(s - 12 * k, 12 * k, 12 * k + 11, s, s + 11, 12)
                                    for k, s in enumerate(REEL_STARTS))
    # (D is reported by neither: not against L, not against R, whose frames it holds in another order)


def mixed_library(seed=41):
    """Reels, a re-cut, a plain excerpt, a full copy, three frames in a row and a shuffled decoy of two long videos."""
    rng = np.random.default_rng(seed)
    L1, L2 = rand(rng, 300), rand(rng, 220)
    reel = AH.noisy(rng, np.concatenate([L1[200:215], L1[30:40], L1[100:103], L1[120:135]]), 20)  # the 3-frame piece never counts
    recut = AH.noisy(rng, np.concatenate([L2[0:50], L2[60:120], L2[121:200]]), 20)
    clip = AH.noisy(rng, L1[50:90], 20)
    copy = AH.noisy(rng, L2, 10)
    decoy = AH.noisy(rng, L1[rng.permutation(300)[:40]], 20)
    return [L1, reel, L2, recut, clip, copy, L1[3:6].copy(), decoy, rand(rng, 25), np.zeros((0, 32), np.uint8)]


def test_keep_rule_floor_and_single_segment_form(hvd):
    from hvd_amd import search

    vids = mixed_library()
    blobs = [v.tobytes() for v in vids]
    got = search.segmented_excerpt_pairs(blobs, matcher=SH.ReferenceMatcher)
    by = {(e.short, e.long): e for e in got}
    # the reel: 15 + 10 + 15 of 43 frames count (93 %), the 3-frame piece does not; segments ordered by short_first
    assert [(s.offset, s.short_first, s.short_last, s.first, s.last, s.aligned) for s in by[(1, 0)].segments] == \
        [(200, 0, 14, 200, 214, 15), (15, 15, 24, 30, 39, 10), (92, 28, 42, 120, 134, 15)]
    assert by[(1, 0)].coverage == 100.0 * 40 / 43
    # the re-cut against its source and against the source's copy; the long video is listed first, so short is b
    for long in (2, 5):
        assert [(s.offset, s.short_first, s.short_last, s.aligned) for s in by[(3, long)].segments] == \
            [(0, 0, 49, 50), (11, 50, 188, 139)]  # votes 60 at 10 and 79 at 11: slack 1 makes them one band
        assert by[(3, long)].coverage == 100.0
    assert [s[:5] for s in by[(4, 0)].segments] == [(50, 0, 39, 50, 89)] and len(by[(2, 5)].segments) == 1
    assert sorted(by) == [(1, 0), (2, 5), (3, 2), (3, 5), (4, 0)]  # no decoy, no three frames in a row
    # min_band_votes = min_aligned (what the entry passes) prunes rounds and changes no result
    assert got == search.segmented_excerpt_pairs(blobs, min_band_votes=1, matcher=SH.ReferenceMatcher)
    for min_aligned in (1, 3, 11):
        assert search.segmented_excerpt_pairs(blobs, 30.0, min_aligned, matcher=SH.ReferenceMatcher) == \
            search.segmented_excerpt_pairs(blobs, 30.0, min_aligned, min_band_votes=1, matcher=SH.ReferenceMatcher)
    assert (6, 0) in {(e.short, e.long) for e in search.segmented_excerpt_pairs(blobs, 50.0, 3, matcher=SH.ReferenceMatcher)}
    # max_segments = 1: the pairs, coverages and offsets of the single-offset search
    for threshold in (20.0, 50.0):
        one = search.segmented_excerpt_pairs(blobs, threshold, max_segments=1, matcher=SH.ReferenceMatcher)
        ref = search.excerpt_pairs(blobs, threshold, matcher=AH.ReferenceMatcher)
        assert [(e.short, e.long, e.coverage, e.similarity) + tuple((s.offset, s.first, s.last) for s in e.segments) for e in one] \
            == [(e.short, e.long, e.coverage, e.similarity, (e.offset, e.first, e.last)) for e in ref] and len(ref) >= 4
    with pytest.raises(ValueError):
        search.segmented_excerpt_pairs(blobs, 0.5, matcher=SH.ReferenceMatcher)
    with pytest.raises(ValueError):
        search.segmented_excerpt_pairs(blobs[:1], positions=[np.arange(3)], matcher=SH.ReferenceMatcher)


def test_reference_dtype_is_the_product_dtype(hvd):
    from hvd_amd import _lib

    assert _lib.VSEGMENTS_DTYPE == SH.VSEGMENTS_DTYPE and _lib.VSEGMENTS_DTYPE.itemsize == 288
    assert _lib.VSEGMENT_DTYPE.itemsize == 32 and _lib.VSEGMENT_DTYPE.names == AH.VALIGN_FIELDS[4:]
    hdr = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert f"#define HVD_ALIGN_MAX_SEGMENTS {_lib.ALIGN_MAX_SEGMENTS}\n" in hdr and _lib.ALIGN_MAX_SEGMENTS == SH.MAX_SEGMENTS
    # the struct of the header, field for field
    seg = re.search(r"typedef struct hvd_vsegment \{(.*?)\} hvd_vsegment;", hdr, re.S).group(1)
    rec = re.search(r"typedef struct hvd_vsegments \{(.*?)\} hvd_vsegments;", hdr, re.S).group(1)

    def names(body):  # "int32_t x, y; uint32_t z[N];" -> ("x", "y", "z")
        decls = [d.split(None, 1)[1] for d in body.split(";") if d.strip()]
        return tuple(re.match(r"\w+", n.strip()).group(0) for d in decls for n in d.split(","))

    assert names(seg) == _lib.VSEGMENT_DTYPE.names
    assert names(rec) == _lib.VSEGMENTS_DTYPE.names and "hvd_vsegment seg[HVD_ALIGN_MAX_SEGMENTS]" in rec
    assert "#define HVD_ABI_VERSION 6 " in hdr


# ---- code shape of the new kernels ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    return _compile("k_valign_segments.hip", str(tmp_path_factory.mktemp("segments_shape")))


def test_lds_form_keeps_its_budget(shapes):
    """DESIGN 4.9 budget of k_valign_segments<false>: no spilled register, no scratch, 256-lane workgroups, LDS and VGPRs for 5
    workgroups per CU (one wave on every SIMD each: 5 waves per SIMD), votes through LDS atomics."""
    k = shapes["k_valign_segments<false>"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and "scratch_" not in k["isa"]
    assert waves_per_simd(k["vgpr"] + k["agpr"]) >= 5, k["vgpr"]
    assert k["wg"] == 256 and 5 * k["lds"] <= LDS_PER_CU, k["lds"]
    assert "ds_add_u32" in k["isa"] and "ds_or_b32" in k["isa"]
    assert "v_bcnt_u32_b32" in k["isa"]  # 8 xor + 8 popcount per comparison


def test_scratch_form_spills_nothing(shapes):
    """The 64 workgroups of k_valign_segments<true> never share a CU's LDS five ways; what must hold is that nothing spills."""
    k = shapes["k_valign_segments<true>"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and "scratch_" not in k["isa"]
    assert k["wg"] == 256 and waves_per_simd(k["vgpr"] + k["agpr"]) >= 4 and 5 * k["lds"] <= LDS_PER_CU
    assert "v_bcnt_u32_b32" in k["isa"]
    assert sorted(shapes) == ["k_valign_segments<false>", "k_valign_segments<true>"]
