"""Time alignment of video pairs on the GPU (run with -m gpu on an MI355X): k_valign and k_kept_positions against
the numpy restatement of the rule (tests/align_helpers.py), record for record and word for word, and the excerpt search end to
end. Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import align_helpers as AH
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

LDS_BINS = 4096  # HVD_ALIGN_LDS_BINS (tests/test_align_cpu.py checks the header against _lib)


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def join(videos):
    off = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)
    fr = np.concatenate(videos) if len(videos) else np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(fr, dtype=np.uint8), off


def same(got, want):
    assert got.dtype == AH.VALIGN_DTYPE and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(got[k].tolist(), want[k].tolist()) for k in bad[:4]]


def dev_align(gpu, fq, oq, pq, ft, ot, pt, pairs, max_dist, slack, scratch_bins):
    """hvd_dev_vpdq_align_videos with its own buffers: records and scratch end in sentinel tails that must stay intact."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    M = pairs.shape[0]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_align_scratch_bytes(scratch_bins, C.byref(sb)))
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(fq=up(fq), oq=up(np.asarray(oq, np.int64)), pq=up(None if pq is None else np.asarray(pq, np.int32)),
                ft=up(ft), ot=up(np.asarray(ot, np.int64)), pt=up(None if pt is None else np.asarray(pt, np.int32)),
                pairs=up(pairs), out=_sentinel_buffer(gpu, 48 * M), scr=_sentinel_buffer(gpu, sb.value) if sb.value else None)
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    try:
        gpu.check(lib.hvd_dev_vpdq_align_videos(ptr("fq"), ptr("oq"), len(oq) - 1, ptr("pq"), ptr("ft"), ptr("ot"), len(ot) - 1,
                                                ptr("pt"), ptr("pairs"), M, max_dist, slack, ptr("scr"), sb.value, ptr("out")))
        gpu.check(lib.hvd_dev_sync())
        out = bufs["out"].to_array(AH.VALIGN_DTYPE, M)
        assert _tail_intact(gpu, bufs["out"], 48 * M), "record buffer overrun"
        assert bufs["scr"] is None or _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return out


def planted_library(seed, max_dist, lengths=(0, 1, 2, 3, 17, 64, 65, 130, 255, 256, 257, 300)):
    """Ragged videos; video v holds a noisy stretch of video v - 1 at a known offset, with frame pairs at exactly max_dist and
    max_dist + 1 both on that diagonal and off it."""
    rng = np.random.default_rng(seed)
    vids = [rand(rng, n) for n in lengths]
    for v in range(1, len(vids)):
        A, B = vids[v - 1], vids[v]
        n = min(len(A), len(B)) // 2
        if n < 1:
            continue
        ia, ib = int(rng.integers(0, len(A) - n + 1)), int(rng.integers(0, len(B) - n + 1))
        B[ib:ib + n] = AH.noisy(rng, A[ia:ia + n], min(max_dist, 24))
        if n >= 4 and max_dist < 127:
            B[ib] = AH.flip_bits(rng, A[ia], max_dist)              # on the diagonal, exactly at the tolerance
            B[ib + 1] = AH.flip_bits(rng, A[ia + 1], max_dist + 1)  # on the diagonal, one past it
            free = [j for j in range(len(B)) if not ib <= j < ib + n]
            if len(free) >= 2:                                      # off the diagonal: at and one past the tolerance
                B[free[0]] = AH.flip_bits(rng, A[ia + 2], max_dist)
                B[free[-1]] = AH.flip_bits(rng, A[ia + 3], max_dist + 1)
    return vids


def gapped_positions(rng, offsets, max_gap=3):
    pos = np.zeros(int(offsets[-1]), np.int32)
    for v in range(len(offsets) - 1):
        n = int(offsets[v + 1] - offsets[v])
        pos[offsets[v]:offsets[v + 1]] = int(rng.integers(0, 50)) + np.cumsum(rng.integers(1, max_gap + 1, n))
    return pos


def all_pairs(V, rng, extra=6):
    pairs = [(a, b) for a in range(V) for b in range(V)]  # a == b and both orders included
    pairs += [pairs[int(k)] for k in rng.integers(0, len(pairs), extra)]  # repeated pairs
    return np.array(pairs, dtype=np.int64)[rng.permutation(len(pairs))]


@pytest.mark.parametrize("max_dist", [0, 30, 31, 32, 127])
@pytest.mark.parametrize("slack", [0, 1, 3, 16])
def test_ragged_libraries_match_the_reference(gpu, hvd, max_dist, slack):
    rng = np.random.default_rng(100 * slack + max_dist)
    frames, offsets = join(planted_library(1000 + max_dist, max_dist))
    pairs = all_pairs(len(offsets) - 1, rng)
    for positions in (None, gapped_positions(rng, offsets)):
        want = AH.align_videos(frames, offsets, pairs, positions, max_dist, slack)
        assert max_dist == 0 or (want["q_aligned"] > 0).sum() > 10
        same(hvd.search.align_videos(frames, offsets, pairs, positions, max_dist, slack), want)
        same(dev_align(gpu, frames, offsets, positions, frames, offsets, positions, pairs, max_dist, slack, 0), want)


def test_static_and_near_static_videos(gpu, hvd):
    """Plateaus of equal S: one image for 50 and 80 frames (the tie order's pinned case), and slowly changing scenes."""
    rng = np.random.default_rng(11)
    h = rand(rng, 1)
    drift = [h[0]]
    for _ in range(299):
        drift.append(AH.flip_bits(rng, drift[-1], 2))  # frames within 15 of each other match: a wide band
    vids = [np.repeat(h, 50, axis=0), np.repeat(h, 80, axis=0), np.array(drift), AH.noisy(rng, np.array(drift[100:180]), 3),
            np.repeat(h, 300, axis=0), AH.noisy(rng, np.repeat(h, 257, axis=0), 12)]
    frames, offsets = join(vids)
    pairs = all_pairs(len(vids), rng)
    for slack in (0, 1, 3, 16):
        want = AH.align_videos(frames, offsets, pairs, None, 31, slack)
        same(hvd.search.align_videos(frames, offsets, pairs, slack=slack), want)
    got = hvd.search.align_videos(frames, offsets, [(0, 1)], slack=1)[0]
    assert got.tolist() == (0, 1, 50, 80, 1, 150, 50, 52, 0, 49, 0, 51)
    assert hvd.Vpdq.align(vids[0].tobytes(), hvd.VpdqHash(vids[1].tobytes())).tolist() == got.tolist()


def switch_case(rng, bins, slack):
    """Two videos whose histogram has exactly `bins` bins: spans 70 and bins - 71 - 2 slack, a planted diagonal (offset 995:
    every second frame of a, up to 31 bits flipped) and strays."""
    A = rand(rng, 40)
    pa = np.sort(rng.choice(np.arange(1, 70), 38, replace=False))
    pa = np.concatenate([[0], pa, [70]]).astype(np.int32) + 5
    span_b = bins - 71 - 2 * slack
    B = rand(rng, 120)
    # b's frames 60..99 sit 995 later than a's frames on their timelines: the planted diagonal
    pb = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 1000), 59, replace=False)), pa + 995,
                         np.sort(rng.choice(np.arange(1100, span_b), 19, replace=False)), [span_b]]).astype(np.int32)
    for k in range(0, 40, 2):
        B[k + 60] = AH.flip_bits(rng, A[k], int(rng.integers(0, 32)))
    B[0], B[119] = A[39], A[0]  # votes in the first and the last bin of the histogram
    return [A, B], np.concatenate([pa, pb])


@pytest.mark.parametrize("slack", [0, 3])
def test_either_side_of_the_lds_scratch_switch(gpu, hvd, slack):
    rng = np.random.default_rng(12 + slack)
    for bins in (LDS_BINS - 1, LDS_BINS, LDS_BINS + 1, LDS_BINS + 2, 3 * LDS_BINS, 1 << 20):
        vids, pos = switch_case(rng, bins, slack)
        frames, offsets = join(vids)
        pairs = [(0, 1), (1, 0), (0, 0)]
        want = AH.align_videos(frames, offsets, pairs, pos, 31, slack)
        assert want[0]["q_aligned"] >= 2 and want[0]["offset"] == -want[1]["offset"]
        same(hvd.search.align_videos(frames, offsets, pairs, pos, slack=slack), want)
        same(dev_align(gpu, frames, offsets, pos, frames, offsets, pos, pairs, 31, slack, bins), want)
        if bins > LDS_BINS:  # no scratch, or too little of it: the INT32_MIN record for the pairs that need it, the others intact
            for scratch_bins in (0, bins // 2):
                got = dev_align(gpu, frames, offsets, pos, frames, offsets, pos, pairs, 31, slack, scratch_bins)
                lost = want.copy()
                for k in (0, 1):
                    lost[k] = (want[k]["a"], want[k]["b"], 0, 0, AH.INT32_MIN, 0, 0, 0, 0, 0, 0, 0)
                same(got, lost)


def test_beyond_the_bin_limit_and_bad_arguments(gpu, hvd):
    rng = np.random.default_rng(13)
    vids, pos = switch_case(rng, (1 << 20) + 1, 0)
    frames, offsets = join(vids)
    got = dev_align(gpu, frames, offsets, pos, frames, offsets, pos, [(0, 1), (0, 0), (0, 2), (7, 0)], 31, 0, 1 << 20)
    want = AH.align_videos(frames, offsets, [(0, 0)], pos, 31, 0)
    assert got[0].tolist() == (0, 1, 0, 0, AH.INT32_MIN, 0, 0, 0, 0, 0, 0, 0)
    assert got[1] == want[0]
    assert got[2].tolist() == (0, 2, 0, 0, AH.INT32_MIN, 0, 0, 0, 0, 0, 0, 0)  # pair index outside [0, V)
    assert got[3].tolist() == (7, 0, 0, 0, AH.INT32_MIN, 0, 0, 0, 0, 0, 0, 0)

    def refused(*args, **kw):
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_videos(*args, **kw)
        assert e.value.code == gpu.HVD_ERR_ARG

    refused(frames, offsets, [(0, 1)], pos, slack=0)            # more than 2^20 bins
    refused(frames, offsets, [(0, 2)])                          # pair index out of range
    refused(frames, offsets, [(0, 1)], slack=17)
    refused(frames, offsets, [(0, 1)], max_dist=128)
    for bad in (-1, 1 << 20):
        p = pos.copy()
        p[3] = bad
        refused(frames, offsets, [(0, 0)], p)
    p = pos.copy()
    p[4] = p[3]                                                 # not strictly increasing
    refused(frames, offsets, [(0, 0)], p)
    refused(frames, np.array([0, 50, 40, 160]), [(0, 1)])       # offsets decrease
    # positions the device entry can see are broken: the INT32_MIN record, nothing out of bounds
    vids, pos = switch_case(rng, 5000, 1)
    frames, offsets = join(vids)
    p = pos.copy()
    p[39] = p[0] + 10                                           # span 10 for 40 frames
    got = dev_align(gpu, frames, offsets, p, frames, offsets, p, [(0, 0), (0, 1), (1, 1)], 31, 1, 10000)
    assert got[0]["offset"] == AH.INT32_MIN and got[1]["offset"] == AH.INT32_MIN
    assert got[2] == AH.align_videos(frames, offsets, [(1, 1)], pos, 31, 1)[0]


def test_empty_list_cross_libraries_and_self_pairs(gpu, hvd):
    rng = np.random.default_rng(14)
    fq, oq = join(planted_library(15, 31, (5, 0, 90, 300)))
    t_vids = planted_library(16, 31, (120, 7, 0, 280, 33))
    q_vids = [fq[oq[v]:oq[v + 1]] for v in range(4)]
    t_vids[0][20:100] = AH.noisy(rng, q_vids[2][5:85], 20)
    t_vids[3][100:280] = AH.noisy(rng, q_vids[3][0:180], 20)
    ft, ot = join(t_vids)
    pq, pt = gapped_positions(rng, oq), gapped_positions(rng, ot, 5)
    pairs = np.array([(a, b) for a in range(4) for b in range(5)] + [(2, 0), (2, 0)], dtype=np.int64)
    for positions in ((None, None), (pq, pt), (pq, None)):
        want = AH.align_videos(fq, oq, pairs, positions[0], 31, 1, ft, ot, positions[1])
        assert positions[0] is not None or want[want["a"] == 2][0]["q_aligned"] >= 70  # (index timelines: the planted stretch)
        same(hvd.search.align_videos(fq, oq, pairs, positions[0], 31, 1, ft, ot, positions[1]), want)
        same(dev_align(gpu, fq, oq, positions[0], ft, ot, positions[1], pairs, 31, 1, 0), want)
    assert hvd.search.align_videos(fq, oq, np.zeros((0, 2), np.int64)).shape == (0,)
    assert dev_align(gpu, fq, oq, None, ft, ot, None, np.zeros((0, 2), np.int64), 31, 1, 0).shape == (0,)
    empty = np.zeros((0, 32), np.uint8)
    same(hvd.search.align_videos(empty, [0, 0], [(0, 0), (0, 0)]), AH.align_videos(empty, [0, 0], [(0, 0), (0, 0)]))
    # VMATCH records as the pair list
    recs = hvd.match_videos(fq, oq, 31)
    same(hvd.search.align_videos(fq, oq, recs), AH.align_videos(fq, oq, np.stack([recs["a"], recs["b"]], axis=1)))


def test_counters_equal_the_video_search(gpu, hvd):
    """Every record of match_videos on a 2000-video library: q_hits / t_hits of the alignment are the hvd_vmatch counters."""
    frames, offsets, _ = hvd.synth.video_hashes(2000, frames_per_video=(0, 96))
    recs = hvd.match_videos(frames, offsets, 31)
    assert len(recs) >= 20
    al = hvd.search.align_videos(frames, offsets, recs)
    for f in ("a", "b", "q_hits", "t_hits"):
        assert np.array_equal(al[f], recs[f]), f
    same(al, AH.align_videos(frames, offsets, np.stack([recs["a"], recs["b"]], axis=1)))
    lib5 = hvd.DeviceLibrary.from_host(frames, offsets)
    try:
        same(lib5.align(recs), al)
    finally:
        lib5.free()


def test_kept_positions_against_numpy(gpu):
    lib = gpu.ensure()
    rng = np.random.default_rng(17)
    small = np.concatenate([[0, 1, 1030, 0, 5], rng.integers(0, 70, 200), [2100]])
    # 1024 * 1024 + 1025 frames: more than one chunk of 1024 block sums, so the scan carries. Ragged lengths with empty
    # videos; video 9001 straddles frame 1024 * 1024.
    n_big = 1024 * 1024 + 1025
    head = np.concatenate([[0, 3, 0, 2000, 1], np.random.default_rng(1717).integers(0, 230, 8996)])
    head[-1] += 1024 * 1024 - 700 - int(head.sum())
    assert head[-1] >= 0 and head.sum() == 1024 * 1024 - 700
    big = np.concatenate([head, [1500, 0, 0, 40], [n_big - 1024 * 1024 - 800 - 40]])
    assert big.sum() == n_big and big[:9001].sum() < 1024 * 1024 < big[:9002].sum() and (big == 0).sum() > 20
    for lengths, dropped in ((small, (2, 4, 9, 10)), (big, (3, 4, 10, 4000, 9004))):
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        n = int(offsets[-1])
        quality = rng.integers(0, 101, n).astype(np.int32)
        for v in dropped:  # videos that lose all their frames
            quality[offsets[v]:offsets[v + 1]] = rng.integers(0, 31, int(lengths[v]))
        for min_q in (31, 0, 101):
            keep = quality >= min_q
            want = (np.arange(n) - np.repeat(offsets[:-1], lengths))[keep].astype(np.int32)
            d_q, d_off = gpu.DeviceBuffer.from_array(quality), gpu.DeviceBuffer.from_array(offsets)
            d_pos = _sentinel_buffer(gpu, 4 * int(keep.sum()))
            try:
                gpu.check(lib.hvd_dev_kept_positions(d_q.ptr, n, d_off.ptr, len(lengths), min_q, d_pos.ptr))
                gpu.check(lib.hvd_dev_sync())
                assert np.array_equal(d_pos.to_array(np.int32, want.size), want)
                assert _tail_intact(gpu, d_pos, 4 * want.size)
            finally:
                for b in (d_q, d_off, d_pos):
                    b.free()


def test_chained_excerpt_search_needs_the_positions(gpu, hvd):
    """Frames in HBM -> hash -> filter -> search -> align. Long videos with constant frames (quality 0: dropped) before and
    inside the stretch a clip was cut from: with the raw positions the clips sit at their raw offsets; on the kept indices
    the offsets come out shifted."""
    S = hvd.synth
    longs = [S.frames_gray(60, seed=21, const_fraction=0.0), S.frames_gray(48, seed=22, const_fraction=0.0)]
    for L, drops in zip(longs, ((3, 4, 9, 25, 26), (0, 30))):
        L[list(drops)] = 77
    vids = [longs[0], longs[0][12:42].copy(), longs[1], longs[1][5:29].copy(), S.frames_gray(20, seed=23)]
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    assert not keep[[3, 4, 9, 25, 26]].any() and keep.sum() >= 60
    # the expectation: the rule on the kept hashes with their raw positions (numpy), which must be the planted clips
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(5)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(5)]
    want = hvd.search.excerpt_pairs(blobs, 50.0, 4, 1, [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(5)],
                                    matcher=AH.ReferenceMatcher)
    assert [(e.short, e.long, e.offset) for e in want] == [(1, 0, 12), (3, 2, 5)]
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        got, recs, aligned, library = hvd.pipeline.find_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, keep_library=True)
        assert got == want
        assert np.array_equal(library.positions(), raw_pos) and np.array_equal(library.offsets(), kept_off)
        library.free()
        same(aligned, AH.align_videos(hashes[keep], kept_off, np.stack([recs["a"], recs["b"]], axis=1), raw_pos))
        shifted, _, _, _ = hvd.pipeline.find_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, positions=False)
        assert [(e.short, e.long) for e in shifted] == [(1, 0), (3, 2)]
        assert [e.offset for e in shifted] != [12, 5]
        assert shifted == hvd.search.excerpt_pairs(blobs, 50.0, 4, 1, None, matcher=AH.ReferenceMatcher)
        assert got == hvd.find_excerpts(blobs, positions=[raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(5)])
    finally:
        d_fr.free()


def test_excerpts_copies_and_distractors_end_to_end(gpu, hvd):
    """A library with planted excerpts, shuffled distractors and full copies: find_excerpts returns the excerpts and the
    copies, find_potential_duplicates (unchanged) only the copies."""
    rng = np.random.default_rng(18)
    vids = [rand(rng, int(n)) for n in rng.integers(20, 60, 30)]
    longs = [rand(rng, n) for n in (400, 300, 240)]
    excerpts, copies = [], []
    for k, L in enumerate(longs):
        at = 60 + 50 * k
        vids.append(L)
        li = len(vids) - 1
        vids.append(AH.noisy(rng, L[at:at + 60], 20))                       # the excerpt
        excerpts.append((li + 1, li, at, at, at + 59))
        vids.append(AH.noisy(rng, L[rng.permutation(len(L))[:60]], 24))     # the same number of frames, no order
        vids.append(AH.noisy(rng, L, 10))                                   # a full copy
        copies.append((li, li + 3))
        excerpts.append((li + 1, li + 3, at, at, at + 59))                  # the excerpt also sits in the copy
    blobs = [v.tobytes() for v in vids]
    got = hvd.find_excerpts(blobs)
    want = sorted(excerpts + [(a, b, 0, 0, len(vids[a]) - 1) for a, b in copies])
    assert [tuple(e[:5]) for e in got] == want
    assert got == hvd.search.excerpt_pairs(blobs, matcher=AH.ReferenceMatcher)
    assert hvd.find_potential_duplicates(blobs) == copies
    by = {(e.short, e.long): e for e in got}
    assert all(int(by[c].similarity) == 100 for c in copies) and all(int(by[e[:2]].similarity) < 50 for e in excerpts)
