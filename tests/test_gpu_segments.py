"""Multi-segment time alignment on the GPU (run with -m gpu on an MI355X): k_valign_segments against the numpy
restatement of the rule (tests/segments_helpers.py), record for record and word for word, against the single-offset kernel, and
the search for reels and re-cuts end to end. Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import align_helpers as AH
import segments_helpers as SH
from test_gpu_align import LDS_BINS, all_pairs, dev_align, gapped_positions, join, planted_library, rand, switch_case
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact
from test_segments_cpu import mixed_library, reel_library

pytestmark = pytest.mark.gpu

REC = SH.VSEGMENTS_DTYPE.itemsize


def dev_segments(gpu, fq, oq, pq, ft, ot, pt, pairs, max_dist, slack, max_segments, min_band_votes, scratch_bins):
    """hvd_dev_vpdq_align_segments with its own buffers: records and scratch end in sentinel tails that must stay intact."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    M = pairs.shape[0]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_segments_scratch_bytes(scratch_bins, C.byref(sb)))
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(fq=up(fq), oq=up(np.asarray(oq, np.int64)), pq=up(None if pq is None else np.asarray(pq, np.int32)),
                ft=up(ft), ot=up(np.asarray(ot, np.int64)), pt=up(None if pt is None else np.asarray(pt, np.int32)),
                pairs=up(pairs), out=_sentinel_buffer(gpu, REC * M), scr=_sentinel_buffer(gpu, sb.value) if sb.value else None)
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    try:
        gpu.check(lib.hvd_dev_vpdq_align_segments(ptr("fq"), ptr("oq"), len(oq) - 1, ptr("pq"), ptr("ft"), ptr("ot"), len(ot) - 1,
                                                  ptr("pt"), ptr("pairs"), M, max_dist, slack, max_segments, min_band_votes,
                                                  ptr("scr"), sb.value, ptr("out")))
        gpu.check(lib.hvd_dev_sync())
        out = bufs["out"].to_array(SH.VSEGMENTS_DTYPE, M)
        assert _tail_intact(gpu, bufs["out"], REC * M), "record buffer overrun"
        assert bufs["scr"] is None or _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return out


@pytest.mark.parametrize("max_dist", [0, 31, 127])
@pytest.mark.parametrize("slack", [0, 1, 3])
def test_planted_pieces_match_the_reference(gpu, hvd, max_dist, slack):
    """The videos of test_gpu_align.planted_library with two to four planted pieces per pair of neighbours; every ordered pair,
    a == b included; index and gapped positions; max_segments 1, 2, 8 x min_band_votes 1, 4; device and host entry."""
    rng = np.random.default_rng(100 * slack + max_dist)
    frames, offsets = join(SH.planted_pieces_library(1000 + max_dist, max_dist))
    pairs = all_pairs(len(offsets) - 1, rng)
    for positions in (None, gapped_positions(rng, offsets)):
        for K in (1, 2, 8):
            for floor in (1, 4):
                want = SH.align_segments(frames, offsets, pairs, positions, max_dist, slack, max_segments=K, min_band_votes=floor)
                if K == 8 and floor == 1 and max_dist:
                    assert (want["n_segments"] >= 2).sum() > 10
                SH.same(dev_segments(gpu, frames, offsets, positions, frames, offsets, positions, pairs, max_dist, slack, K, floor,
                                     0), want)
                SH.same(hvd.search.align_segments(frames, offsets, pairs, positions, max_dist, slack, max_segments=K,
                                                  min_band_votes=floor), want)


def test_separate_target_library_empty_list_and_static_videos(gpu, hvd):
    rng = np.random.default_rng(14)
    fq, oq = join(planted_library(15, 31, (5, 0, 90, 300)))
    t_vids = SH.planted_pieces_library(16, 31, (120, 7, 0, 280, 33))
    q_vids = [fq[oq[v]:oq[v + 1]] for v in range(4)]
    t_vids[0][20:60] = AH.noisy(rng, q_vids[2][5:45], 20)      # two pieces of query 2 in target 0
    t_vids[0][70:100] = AH.noisy(rng, q_vids[2][60:90], 20)
    t_vids[3][0:100] = AH.noisy(rng, q_vids[3][150:250], 20)   # query 3 re-cut into target 3
    t_vids[3][100:220] = AH.noisy(rng, q_vids[3][0:120], 20)
    ft, ot = join(t_vids)
    pq, pt = gapped_positions(rng, oq), gapped_positions(rng, ot, 5)
    pairs = np.array([(a, b) for a in range(4) for b in range(5)] + [(2, 0), (2, 0)], dtype=np.int64)
    for positions in ((None, None), (pq, pt), (pq, None)):
        want = SH.align_segments(fq, oq, pairs, positions[0], 31, 1, ft, ot, positions[1])
        if positions[0] is None:
            by = {(int(r["a"]), int(r["b"])): r for r in want}
            assert by[(2, 0)]["seg"]["offset"][:2].tolist() == [15, 10] and by[(3, 3)]["seg"]["offset"][:2].tolist() == [100, -150]
        SH.same(hvd.search.align_segments(fq, oq, pairs, positions[0], 31, 1, ft, ot, positions[1]), want)
        SH.same(dev_segments(gpu, fq, oq, positions[0], ft, ot, positions[1], pairs, 31, 1, 8, 1, 0), want)
    assert hvd.search.align_segments(fq, oq, np.zeros((0, 2), np.int64)).shape == (0,)
    assert dev_segments(gpu, fq, oq, None, ft, ot, None, np.zeros((0, 2), np.int64), 31, 1, 8, 1, 0).shape == (0,)
    empty = np.zeros((0, 32), np.uint8)
    SH.same(hvd.search.align_segments(empty, [0, 0], [(0, 0), (0, 0)]), SH.align_segments(empty, [0, 0], [(0, 0), (0, 0)]))
    # the pinned static case: one segment, then every frame of a is taken
    h = rand(rng, 1)
    vids = [np.repeat(h, 50, axis=0), np.repeat(h, 80, axis=0), AH.noisy(rng, np.repeat(h, 257, axis=0), 12)]
    frames, offsets = join(vids)
    pairs = all_pairs(3, rng)
    for slack in (0, 1, 3, 16):
        SH.same(hvd.search.align_segments(frames, offsets, pairs, slack=slack), SH.align_segments(frames, offsets, pairs, slack=slack))
    got = hvd.search.align_segments(frames, offsets, [(0, 1)])[0]
    assert got.tolist()[:8] == (0, 1, 50, 80, 1, 50, 52, 0) and got["seg"][0].tolist() == (1, 150, 50, 52, 0, 49, 0, 51)
    assert got["seg"][1:].tobytes() == bytes(7 * 32)
    assert hvd.Vpdq.align_segments(vids[0].tobytes(), hvd.VpdqHash(vids[1].tobytes())) == got


@pytest.mark.parametrize("slack", [0, 3])
def test_either_side_of_the_lds_scratch_switch(gpu, hvd, slack):
    """Pairs beyond HVD_ALIGN_LDS_BINS: exact with scratch; without scratch, or with too small a slot, the INT32_MIN record."""
    rng = np.random.default_rng(12 + slack)
    for bins in (LDS_BINS, LDS_BINS + 1, 3 * LDS_BINS, 1 << 20):
        vids, pos = switch_case(rng, bins, slack)
        frames, offsets = join(vids)
        pairs = [(0, 1), (1, 0), (0, 0)]
        want = SH.align_segments(frames, offsets, pairs, pos, 31, slack)
        assert want[0]["n_segments"] >= 2 and want[0]["seg"][0]["offset"] == -want[1]["seg"][0]["offset"]
        SH.same(hvd.search.align_segments(frames, offsets, pairs, pos, slack=slack), want)
        SH.same(dev_segments(gpu, frames, offsets, pos, frames, offsets, pos, pairs, 31, slack, 8, 1, bins), want)
        if bins > LDS_BINS:
            for scratch_bins in (0, bins // 2):
                got = dev_segments(gpu, frames, offsets, pos, frames, offsets, pos, pairs, 31, slack, 8, 1, scratch_bins)
                lost = want.copy()
                for k in (0, 1):
                    lost[k] = SH.lost_record(want[k]["a"], want[k]["b"])
                SH.same(got, lost)


def test_invalid_input(gpu, hvd):
    rng = np.random.default_rng(13)
    vids, pos = switch_case(rng, (1 << 20) + 1, 0)
    frames, offsets = join(vids)
    got = dev_segments(gpu, frames, offsets, pos, frames, offsets, pos, [(0, 1), (0, 0), (0, 2), (7, 0)], 31, 0, 8, 1, 1 << 20)
    assert got[0] == SH.lost_record(0, 1)                       # more than 2^20 bins
    assert got[1] == SH.align_segments(frames, offsets, [(0, 0)], pos, 31, 0)[0]
    assert got[2] == SH.lost_record(0, 2) and got[3] == SH.lost_record(7, 0)  # pair index outside [0, V)
    # positions the device entry can see are broken: the INT32_MIN record, nothing out of bounds
    vids5, pos5 = switch_case(rng, 5000, 1)
    frames5, offsets5 = join(vids5)
    p = pos5.copy()
    p[39] = p[0] + 10                                           # span 10 for 40 frames
    got = dev_segments(gpu, frames5, offsets5, p, frames5, offsets5, p, [(0, 0), (0, 1), (1, 1)], 31, 1, 8, 1, 10000)
    assert got[0] == SH.lost_record(0, 0) and got[1] == SH.lost_record(0, 1)
    assert got[2] == SH.align_segments(frames5, offsets5, [(1, 1)], pos5, 31, 1)[0]

    def refused(*args, **kw):
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_segments(*args, **kw)
        assert e.value.code == gpu.HVD_ERR_ARG

    refused(frames, offsets, [(0, 1)], pos, slack=0)            # more than 2^20 bins
    refused(frames, offsets, [(0, 2)])                          # pair index out of range
    refused(frames, offsets, [(0, 1)], slack=17)
    refused(frames, offsets, [(0, 1)], max_dist=128)
    for K in (0, 9):
        refused(frames, offsets, [(0, 0)], max_segments=K)
    refused(frames, offsets, [(0, 0)], min_band_votes=0)
    for bad in (-1, 1 << 20):
        p = pos.copy()
        p[3] = bad
        refused(frames, offsets, [(0, 0)], p)
    p = pos.copy()
    p[4] = p[3]                                                 # not strictly increasing
    refused(frames, offsets, [(0, 0)], p)
    refused(frames, np.array([0, 50, 40, 160]), [(0, 1)])       # offsets decrease
    # the device entry refuses the arguments it can check without the device
    lib = gpu.ensure()
    d = gpu.DeviceBuffer(4096)
    try:
        for K, floor in ((0, 1), (9, 1), (8, 0)):
            assert lib.hvd_dev_vpdq_align_segments(d.ptr, d.ptr, 1, None, d.ptr, d.ptr, 1, None, d.ptr, 1, 31, 1, K, floor, None, 0,
                                                   d.ptr) == gpu.HVD_ERR_ARG
    finally:
        d.free()


def test_one_segment_is_the_single_offset_kernel(gpu, hvd):
    """max_segments 1: the record's leading words and seg[0] are the hvd_dev_vpdq_align_videos record of the same call."""
    rng = np.random.default_rng(19)
    frames, offsets = join(SH.planted_pieces_library(1031, 31))
    pairs = all_pairs(len(offsets) - 1, rng)
    for positions, slack in ((None, 1), (gapped_positions(rng, offsets), 3)):
        one = dev_segments(gpu, frames, offsets, positions, frames, offsets, positions, pairs, 31, slack, 1, 1, 0)
        ref = dev_align(gpu, frames, offsets, positions, frames, offsets, positions, pairs, 31, slack, 0)
        assert (ref["q_aligned"] > 0).sum() > 10
        for f in ("a", "b", "q_hits", "t_hits"):
            assert np.array_equal(one[f], ref[f]), f
        for f in SH.VSEGMENT_DTYPE.names:
            assert np.array_equal(one["seg"][f][:, 0], ref[f]), f
        assert np.array_equal(one["n_segments"], (ref["q_aligned"] > 0).astype(np.uint32))
        assert np.array_equal(one["q_covered"], ref["q_aligned"]) and np.array_equal(one["t_covered"], ref["t_aligned"])
        assert not one["seg"][:, 1:].tobytes().strip(b"\0")
    # all eight segments: seg[0] stays that record
    many = dev_segments(gpu, frames, offsets, None, frames, offsets, None, pairs, 31, 1, 8, 1, 0)
    ref = dev_align(gpu, frames, offsets, None, frames, offsets, None, pairs, 31, 1, 0)
    for f in SH.VSEGMENT_DTYPE.names:
        assert np.array_equal(many["seg"][f][:, 0], ref[f]), f


@pytest.mark.parametrize("n", [2040, 3000])
def test_one_long_pair_with_four_planted_pieces(gpu, hvd, n):
    """2 040 frames a side: 4 081 bins, the LDS form over eight chunks of video a; 3 000 a side: 6 001 bins, the scratch form."""
    rng = np.random.default_rng(n)
    A, B = rand(rng, n), rand(rng, n)
    planted = ((100, 1500, 400), (900, 200, 300), (1400, 1000, 250), (1800, 1900, 100))  # (start in a, start in b, frames)
    for ia, ib, m in planted:
        B[ib:ib + m] = AH.noisy(rng, A[ia:ia + m], 24)
    frames, offsets = join([A, B])
    pairs = [(0, 1), (1, 0)]
    want = SH.align_segments(frames, offsets, pairs)
    assert want[0]["seg"]["offset"][:4].tolist() == [ib - ia for ia, ib, m in planted]
    assert want[0]["seg"]["q_aligned"][:4].tolist() == [m for ia, ib, m in planted] and want[0]["n_segments"] == 4
    SH.same(hvd.search.align_segments(frames, offsets, pairs), want)
    lib5 = hvd.DeviceLibrary.from_host(frames, offsets)
    try:
        SH.same(lib5.align_segments(pairs), want)
        SH.same(lib5.align_segments(pairs, max_segments=3, min_band_votes=200),
                SH.align_segments(frames, offsets, pairs, max_segments=3, min_band_votes=200))
    finally:
        lib5.free()


def test_reels_recuts_copies_and_decoys_end_to_end(gpu, hvd):
    """find_segmented_excerpts on the GPU is the rule on the restatement; find_excerpts on the same library misses the reels."""
    vids = mixed_library() + reel_library()
    blobs = [v.tobytes() for v in vids]
    got = hvd.find_segmented_excerpts(blobs)
    assert got == hvd.search.segmented_excerpt_pairs(blobs, matcher=SH.ReferenceMatcher)
    found = {(e.short, e.long): len(e.segments) for e in got}
    assert found == {(1, 0): 3, (2, 5): 1, (3, 2): 2, (3, 5): 2, (4, 0): 1, (11, 10): 5}  # no decoy (7), no shuffled reel (12)
    single = {(e.short, e.long) for e in hvd.find_excerpts(blobs)}
    assert single == set(found) - {(1, 0), (11, 10)}
    assert hvd.find_excerpts(blobs) == hvd.search.excerpt_pairs(blobs, matcher=AH.ReferenceMatcher)
    # max_segments 1 is find_excerpts; min_band_votes 1 changes nothing
    one = hvd.find_segmented_excerpts(blobs, max_segments=1)
    assert [(e.short, e.long, e.coverage, e.segments[0].offset, e.segments[0].first, e.segments[0].last) for e in one] == \
        [(e.short, e.long, e.coverage, e.offset, e.first, e.last) for e in hvd.find_excerpts(blobs)]
    assert got == hvd.search.segmented_excerpt_pairs(blobs, min_band_votes=1)
    for kw in (dict(threshold=20.0, min_aligned=3), dict(slack=0), dict(max_segments=2)):
        assert hvd.find_segmented_excerpts(blobs, **kw) == hvd.search.segmented_excerpt_pairs(blobs, matcher=SH.ReferenceMatcher,
                                                                                              **kw)


def test_chained_search_for_a_reel_needs_the_positions(gpu, hvd):
    """Frames in HBM -> hash -> filter -> search -> segment alignment. The long video has constant frames (quality 0: dropped)
    before and inside the pieces the reel was cut from: with the raw positions the pieces sit at their raw offsets."""
    S = hvd.synth
    long = S.frames_gray(70, seed=21, const_fraction=0.0)
    long[[3, 4, 9, 27, 28, 45]] = 77
    reel = np.concatenate([long[40:52], long[5:17], long[24:36]])  # raw offsets 40, -7, 0
    vids = [long, reel, S.frames_gray(20, seed=23)]
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    assert not keep[[3, 4, 9, 27, 28, 45]].any() and keep[:70].sum() >= 40
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(3)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(3)]
    positions = [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(3)]
    want = hvd.search.segmented_excerpt_pairs(blobs, positions=positions, matcher=SH.ReferenceMatcher)
    assert [(e.short, e.long) for e in want] == [(1, 0)] and [s.offset for s in want[0].segments] == [40, -7, 0]
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        got, recs, aligned, library = hvd.pipeline.find_segmented_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, keep_library=True)
        assert got == want
        assert np.array_equal(library.positions(), raw_pos) and np.array_equal(library.offsets(), kept_off)
        library.free()
        SH.same(aligned, SH.align_segments(hashes[keep], kept_off, np.stack([recs["a"], recs["b"]], axis=1), raw_pos,
                                           min_band_votes=4))
        assert got == hvd.find_segmented_excerpts(blobs, positions=positions)
        shifted, _, _, _ = hvd.pipeline.find_segmented_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, positions=False)
        assert shifted == hvd.search.segmented_excerpt_pairs(blobs, matcher=SH.ReferenceMatcher)
        assert [s.offset for e in shifted for s in e.segments] != [40, -7, 0]
    finally:
        d_fr.free()
