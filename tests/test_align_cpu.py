"""Excerpt search without a GPU: the numpy restatement of the alignment rule (tests/align_helpers.py) gives the
hand-derived records; the premise of the feature holds on it -- the vPDQ counters cannot tell an excerpt from the same frames
in shuffled order, the alignment can; the new kernels compile for gfx950 without spills or scratch."""
import os
import shutil

import numpy as np
import pytest

import align_helpers as AH
from conftest import ROOT
from test_code_shape import HIPCC, LDS_PER_CU, _compile, waves_per_simd


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


# ---- the rule, on hand-derived cases ----

def test_static_videos_pin_the_tie_order():
    """50 frames against 80 frames of one image: votes[d] = 50 for d in 0..30, S = 150 for d in 1..29 under slack 1; equal S
    and equal votes leave the smallest |d|: 1. Frames of b within 1 of that diagonal: j - i in {0, 1, 2} -> j in 0..51."""
    h = rand(np.random.default_rng(1), 1)
    A, B = np.repeat(h, 50, axis=0), np.repeat(h, 80, axis=0)
    assert AH.align_pair(A, B, slack=1) == (50, 80, 1, 150, 50, 52, 0, 49, 0, 51)
    # slack 0: votes = S = 50 for d in 0..30 -> d* = 0, and only j = i is on it
    assert AH.align_pair(A, B, slack=0) == (50, 80, 0, 50, 50, 50, 0, 49, 0, 49)
    # the other way round the diagonals are negative: S = 150 for d in -29..-1 -> d* = -1
    assert AH.align_pair(B, A, slack=1) == (80, 50, -1, 150, 52, 50, 0, 51, 0, 49)


@pytest.mark.parametrize("slack", [0, 1, 2, 3])
def test_single_planted_diagonal(slack):
    """10 frames copied to b at offset 7: the window sums tie at 10 for d in 7 - slack .. 7 + slack, votes[7] = 10 decides."""
    rng = np.random.default_rng(2)
    A, B = rand(rng, 10), rand(rng, 30)
    B[7:17] = A
    assert AH.align_pair(A, B, slack=slack) == (10, 10, 7, 10, 10, 10, 0, 9, 7, 16)


def test_two_diagonals_with_equal_sums_follow_the_tie_order():
    rng = np.random.default_rng(3)
    # equal S, equal votes: the smaller |d| (-3 against +5)
    A, B = rand(rng, 8), rand(rng, 20)
    B[5:9] = A[0:4]   # d = +5
    B[1:5] = A[4:8]   # d = -3
    assert AH.align_pair(A, B, slack=0) == (8, 8, -3, 4, 4, 4, 4, 7, 1, 4)
    # equal S, votes and |d|: the smaller d (-4 against +4)
    A, B = rand(rng, 8), rand(rng, 20)
    B[4:7] = A[0:3]   # d = +4
    B[1:4] = A[5:8]   # d = -4
    assert AH.align_pair(A, B, slack=0) == (6, 6, -4, 3, 3, 3, 5, 7, 1, 3)
    # equal S: the larger votes[d] wins although its |d| is larger. d = 2 three times and d = 3 once: S(2) = S(3) = 4 with
    # votes 3 and 1; d = 9 four times: S(8) = S(9) = S(10) = 4 with votes[9] = 4
    A, B = rand(rng, 12), rand(rng, 24)
    B[2:5] = A[0:3]
    B[6] = A[3]
    B[13:17] = A[4:8]
    assert AH.align_pair(A, B, slack=1) == (8, 8, 9, 4, 4, 4, 4, 7, 13, 16)


def test_no_hit_and_empty_videos_give_the_zero_record():
    rng = np.random.default_rng(4)
    A, B = rand(rng, 12), rand(rng, 9)
    assert AH.hamming_matrix(A, B).min() > 31
    assert AH.align_pair(A, B) == (0,) * 10
    assert AH.align_pair(A[:0], B) == (0,) * 10 and AH.align_pair(A, B[:0]) == (0,) * 10
    recs = AH.align_videos(np.concatenate([A, B]), [0, 12, 12, 21], [(0, 2), (1, 2), (0, 1)])
    assert recs.tolist() == [(0, 2) + (0,) * 10, (1, 2) + (0,) * 10, (0, 1) + (0,) * 10]


def test_given_positions_with_gaps():
    """Frames 0, 2, 3 of a sit 10 later in b's timeline, two more hits lie elsewhere (13, 23). On the frame indices instead the
    same hits read 0, 0, 0, 0, 1: another offset and a band that swallows a stray hit -- the positions matter."""
    rng = np.random.default_rng(5)
    A, B = rand(rng, 5), rand(rng, 6)
    pa, pb = [0, 2, 3, 7, 8], [10, 12, 13, 20, 30, 31]
    B[0], B[1], B[2], B[3], B[5] = A[0], A[1], A[2], A[3], A[4]
    assert AH.align_pair(A, B, pa, pb, slack=1) == (5, 5, 10, 3, 3, 3, 0, 3, 10, 13)
    assert AH.align_pair(A, B, pa, pb, slack=3) == (5, 5, 10, 4, 4, 4, 0, 7, 10, 20)
    assert AH.align_pair(A, B, slack=1) == (5, 5, 0, 5, 5, 5, 0, 4, 0, 5)


def test_tolerance_edge_is_inclusive():
    rng = np.random.default_rng(6)
    A = rand(rng, 3)
    B = np.stack([AH.flip_bits(rng, A[0], 31), AH.flip_bits(rng, A[1], 32), A[2]])
    assert AH.align_pair(A, B, max_dist=31, slack=0) == (2, 2, 0, 2, 2, 2, 0, 2, 0, 2)
    assert AH.align_pair(A, B, max_dist=32, slack=0) == (3, 3, 0, 3, 3, 3, 0, 2, 0, 2)


# ---- the premise: counters cannot tell an excerpt from a shuffle, the alignment can ----

def premise_library(seed=7):
    """L: 600 frames. E: frames 200..259 of L, up to 24 bits flipped. D: 60 frames of L in shuffled order, same flips."""
    rng = np.random.default_rng(seed)
    L = rand(rng, 600)
    E = AH.noisy(rng, L[200:260], 24)
    D = AH.noisy(rng, L[rng.permutation(600)[:60]], 24)
    return [L, E, D]


def test_premise_counters_are_blind_and_alignment_is_not(hvd):
    from hvd_amd import search

    vids = premise_library()
    frames = np.concatenate(vids)
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    lengths = np.diff(offsets)
    recs = AH.ReferenceMatcher.match_videos(frames, offsets, 31)
    by = {(int(r["a"]), int(r["b"])): r for r in recs}
    assert (by[(0, 1)]["t_hits"], by[(0, 2)]["t_hits"]) == (60, 60)  # every frame of E and of D hits L
    # "min": the excerpt scores 10 and is never reported; "max": it is, and so is the shuffled distractor
    sim_min = search.similarity_of_records(recs, lengths, "min")
    sim_max = search.similarity_of_records(recs, lengths, "max")
    where = {(int(r["a"]), int(r["b"])): k for k, r in enumerate(recs)}
    assert int(sim_min[where[(0, 1)]]) == 10 and int(sim_min[where[(0, 2)]]) == 10
    assert search.similar_video_pairs(recs, lengths, 50.0, "min").tolist() == []
    assert [0, 1] in search.similar_video_pairs(recs, lengths, 50.0, "max").tolist()
    assert [0, 2] in search.similar_video_pairs(recs, lengths, 50.0, "max").tolist()
    # the alignment: E sits at offset 200 with all 60 frames on it, D has a handful
    al = AH.align_videos(frames, offsets, [(1, 0), (2, 0)])
    assert (al[0]["offset"], al[0]["q_aligned"], al[0]["t_first"], al[0]["t_last"]) == (200, 60, 200, 259)
    assert al[1]["q_hits"] == 60 and al[1]["q_aligned"] < 30
    # find_excerpts' rule on the reference keeps E and drops D
    blobs = [v.tobytes() for v in vids]
    got = search.excerpt_pairs(blobs, 50.0, 4, 1, None, matcher=AH.ReferenceMatcher)
    assert [tuple(e[:5]) for e in got] == [(1, 0, 200, 200, 259)]
    assert got[0].coverage == 100.0 and int(got[0].similarity) == 10


def test_excerpt_rule_orientation_thresholds_and_full_copies(hvd):
    from hvd_amd import search

    rng = np.random.default_rng(8)
    L = rand(rng, 40)
    copy = AH.noisy(rng, L, 15)           # a full copy: similarity 100 and coverage 100
    clip = AH.noisy(rng, L[25:37], 15)    # 12 frames of L from 25 on, listed BEFORE the long video
    three = L[3:6].copy()                 # three frames in a row: below min_aligned
    blobs = [clip.tobytes(), L.tobytes(), copy.tobytes(), three.tobytes(), b""]
    got = search.excerpt_pairs(blobs, 50.0, 4, 1, None, matcher=AH.ReferenceMatcher)
    assert [tuple(e[:5]) for e in got] == [(0, 1, 25, 25, 36), (0, 2, 25, 25, 36), (1, 2, 0, 0, 39)]
    assert [int(e.similarity) for e in got] == [30, 30, 100]
    got3 = search.excerpt_pairs(blobs, 50.0, 3, 1, None, matcher=AH.ReferenceMatcher)
    assert (3, 1, 3, 3, 5) in [tuple(e[:5]) for e in got3]
    # the long video listed first: short is b, the offset is reported in the long video's timeline all the same
    got = search.excerpt_pairs([L.tobytes(), clip.tobytes()], 50.0, 4, 1, None, matcher=AH.ReferenceMatcher)
    assert [tuple(e[:5]) for e in got] == [(1, 0, 25, 25, 36)]
    # positions: L hashed every second raw frame, the clip every raw frame of the same stretch
    pos = [np.arange(40) * 2, np.arange(50, 74)]
    clip2 = np.repeat(L[25:37], 2, axis=0)
    got = search.excerpt_pairs([L.tobytes(), clip2.tobytes()], 50.0, 4, 1, pos, matcher=AH.ReferenceMatcher)
    assert [tuple(e[:5]) for e in got] == [(1, 0, 0, 50, 72)]
    with pytest.raises(ValueError):
        search.excerpt_pairs(blobs, 0.5, 4, 1, None, matcher=AH.ReferenceMatcher)
    with pytest.raises(ValueError):
        search.excerpt_pairs([L.tobytes()], 50.0, 4, 1, [np.arange(3)], matcher=AH.ReferenceMatcher)


def test_reference_dtype_is_the_product_dtype(hvd):
    from hvd_amd import _lib

    assert _lib.VALIGN_DTYPE == AH.VALIGN_DTYPE and _lib.VALIGN_DTYPE.itemsize == 48
    hdr = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert f"#define HVD_ALIGN_LDS_BINS {_lib.ALIGN_LDS_BINS}\n" in hdr


# ---- code shape of the new kernels ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    tmp = str(tmp_path_factory.mktemp("align_shape"))
    return {"valign": _compile("k_valign.hip", tmp), "vmatch": _compile("k_vmatch.hip", tmp)}


@pytest.mark.parametrize("name", ["k_valign<false>", "k_valign<true>"])
def test_align_kernels_spill_nothing(shapes, name):
    """DESIGN 4.8 budget: no spilled register, no scratch; LDS for 5 workgroups per CU (a 256-lane workgroup puts one wave
    on every SIMD, so that is 5 waves per SIMD) and VGPRs that do not lower that."""
    k = shapes["valign"][name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and "scratch_" not in k["isa"]
    assert waves_per_simd(k["vgpr"]) >= 5, k["vgpr"]
    assert k["wg"] == 256 and 5 * k["lds"] <= LDS_PER_CU, k["lds"]
    assert "ds_add_u32" in k["isa"] or name == "k_valign<true>"  # the LDS form votes with LDS atomics
    assert "v_bcnt_u32_b32" in k["isa"]  # 8 xor + 8 popcount per comparison


def test_kept_positions_kernel_spills_nothing(shapes):
    k = shapes["vmatch"]["k_kept_positions"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0
    assert waves_per_simd(k["vgpr"]) == 8

