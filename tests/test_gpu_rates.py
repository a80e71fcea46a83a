"""Rate-aware time alignment on the GPU (run with -m gpu on an MI355X): k_valign_rates against the numpy
restatement of the rule (tests/rates_helpers.py), record for record and word for word, through the host entry, the device entry
and the chained pipeline. Every comparison is equality."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import align_helpers as AH
import rates_helpers as RH
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

LDS_BINS = 4096   # HVD_ALIGN_LDS_BINS
LDS_GRID = 8192   # workgroups of the LDS launch at most (launch_lds_then_scratch)
SLOTS = 64        # workgroups of the scratch launch, one slot of the scratch each


def rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def same(got, want):
    assert got.dtype == RH.VRATE_DTYPE and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(got[k].tolist(), want[k].tolist()) for k in bad[:4]]


def bins_of(na_span, nb_span, rates, slack):
    return max(n * na_span + d * nb_span + 1 + 2 * slack * max(n, d) for n, d in rates)


def dev_rates(gpu, fq, oq, pq, ft, ot, pt, pairs, rates, max_dist=31, slack=1, scratch_bins=0, scratch_bytes=None):
    """hvd_dev_vpdq_align_rates with its own buffers: records and scratch end in sentinel tails that must stay intact.
    scratch_bytes: what the entry is TOLD it has (the buffer itself is sized for scratch_bins)."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    rates = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
    M = pairs.shape[0]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_rates_scratch_bytes(scratch_bins, C.byref(sb)))
    told = sb.value if scratch_bytes is None else scratch_bytes
    assert told <= sb.value
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(fq=up(fq), oq=up(np.asarray(oq, np.int64)), pq=up(None if pq is None else np.asarray(pq, np.int32)),
                ft=up(ft), ot=up(np.asarray(ot, np.int64)), pt=up(None if pt is None else np.asarray(pt, np.int32)),
                pairs=up(pairs), out=_sentinel_buffer(gpu, 64 * M), scr=_sentinel_buffer(gpu, sb.value) if sb.value else None)
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    try:
        gpu.check(lib.hvd_dev_vpdq_align_rates(ptr("fq"), ptr("oq"), len(oq) - 1, ptr("pq"), ptr("ft"), ptr("ot"), len(ot) - 1,
                                               ptr("pt"), ptr("pairs"), M, max_dist, slack, rates.ctypes.data, rates.shape[0],
                                               ptr("scr"), told, ptr("out")))
        gpu.check(lib.hvd_dev_sync())
        out = bufs["out"].to_array(RH.VRATE_DTYPE, M)
        assert _tail_intact(gpu, bufs["out"], 64 * M), "record buffer overrun"
        assert bufs["scr"] is None or _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return out


@pytest.fixture(scope="module")
def planted():
    """The 600-frame source, its seven 60-frame clips (up to 20 bits flipped), and the restatement's records of every clip
    against the source in both orientations, under the default list and under the list that holds (1, 2)."""
    source, clips = RH.planted_clips(seed=74, max_flips=20)
    frames, offsets = RH.join([source] + [clips[r] for r in RH.PLANTED_RATES])
    pairs = [(v, 0) for v in range(1, 8)] + [(0, v) for v in range(1, 8)]
    lists = (RH.DEFAULT_RATES, RH.list_with((1, 2)))
    want = [RH.align_rates(frames, offsets, pairs, None, rates) for rates in lists]
    return frames, offsets, pairs, lists, want


def test_planted_rates_in_both_orientations(gpu, hvd, planted):
    frames, offsets, pairs, lists, wants = planted
    for rates, want in zip(lists, wants):
        assert bins_of(599, 59, rates, 1) <= 3242 <= LDS_BINS and bins_of(59, 599, rates, 1) <= 3242  # the LDS form
        for k, rate in enumerate(RH.PLANTED_RATES):  # 60 of 60 at the planted rate; as b: at its inverse
            if rate in rates:
                assert want[k].tolist()[5:8] == (60, 60, len(set(want_idx(rate)))) and want[k].tolist()[12:14] == rate
            if rate[::-1] in rates:
                assert want[7 + k]["band_votes"] == 60 and want[7 + k]["t_aligned"] == 60 and want[7 + k].tolist()[12:14] == rate[::-1]
                assert rate not in rates or want[7 + k]["offset"] == -want[k]["offset"]
        same(hvd.search.align_rates(frames, offsets, pairs, rates=rates), want)
        same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, rates), want)
    rec = hvd.Vpdq.align_rates(frames[offsets[1]:offsets[2]].tobytes(), hvd.VpdqHash(frames[:600].tobytes()))
    assert rec.tolist()[2:] == wants[0][0].tolist()[2:] and (rec["a"], rec["b"]) == (0, 1)


def want_idx(rate):
    return np.floor(np.arange(60) * rate[0] / rate[1] + 100.3 + 0.5).astype(np.int64).tolist()


def test_unit_list_is_the_single_offset_alignment(gpu, hvd):
    """rates = [(1, 1)] on a mixed pair list: words 0-11 are search.align_videos' records of the same list, words 12-15 are
    1, 1, 0, 0 (0 for a pair without a hit)."""
    rng = np.random.default_rng(61)
    frames, offsets = RH.join(RH.mixed_library(61))
    V = len(offsets) - 1
    pairs = np.array([(a, b) for a in range(V) for b in range(V)], dtype=np.int64)[rng.permutation(V * V)]
    for slack in (0, 1, 3):
        single = hvd.search.align_videos(frames, offsets, pairs, slack=slack)
        got = hvd.search.align_rates(frames, offsets, pairs, rates=((1, 1),), slack=slack)
        for s, g in zip(single, got):
            assert g.tolist()[:12] == s.tolist()
            assert g.tolist()[12:] == ((1, 1, 0, 0) if s["q_hits"] else (0, 0, 0, 0))
        same(got, RH.align_rates(frames, offsets, pairs, None, ((1, 1),), slack))
    # the whole list on the same pairs, and the counters and the (1, 1) band as the header states them
    full = hvd.search.align_rates(frames, offsets, pairs)
    same(full, RH.align_rates(frames, offsets, pairs))
    single = hvd.search.align_videos(frames, offsets, pairs)
    assert np.array_equal(full["q_hits"], single["q_hits"]) and np.array_equal(full["t_hits"], single["t_hits"])
    assert (full["band_votes"] >= single["band_votes"]).all() and (full["rate_index"] > 0).sum() >= 8


def test_chunk_and_lane_split_edges(gpu, hvd):
    """na in {1, 255, 256, 257, 513} (the 256-frame chunks of video a) against nb in {1, 3, 255, 256, 257} (one frame of b per
    lane; short b sides dealt over 256 // nb lanes): a is a prefix of one source, b runs through it at 5/4, so that the hits of
    a pair end where a ends. Index positions and positions with gaps."""
    rng = np.random.default_rng(62)
    S = rand(rng, 513)
    a_vids = [S[:n].copy() for n in (1, 255, 256, 257, 513)]
    b_vids = [AH.noisy(rng, RH.resampled(S, n, 5, 4, 0.3), 20) for n in (1, 3, 255, 256, 257)]
    fq, oq = RH.join(a_vids)
    ft, ot = RH.join(b_vids)
    pairs = [(a, b) for a in range(5) for b in range(5)]
    gaps = lambda off: np.concatenate([int(rng.integers(0, 5)) + np.cumsum(rng.integers(1, 3, int(n)))  # noqa: E731
                                       for n in np.diff(off)]).astype(np.int32)
    for pq, pt, slack in ((None, None, 1), (gaps(oq), gaps(ot), 2)):
        want = RH.align_rates(fq, oq, pairs, pq, RH.DEFAULT_RATES, slack, 31, ft, ot, pt)
        assert (want["q_hits"] > 0).all()
        if pq is None:  # b at 5/4 of a: p_b = 4/5 p_a; 257 frames of b reach source index 320
            assert want[24].tolist()[12:14] == (4, 5) and want[24]["t_aligned"] == 257 and want[9]["t_aligned"] >= 200
            assert max(bins_of(512, 256, RH.DEFAULT_RATES, 1), bins_of(256, 512, RH.DEFAULT_RATES, 1)) <= LDS_BINS
        same(hvd.search.align_rates(fq, oq, pairs, pq, RH.DEFAULT_RATES, slack, None, ft, ot, pt), want)
        big = bins_of(int(2 * 513), int(2 * 257), RH.DEFAULT_RATES, slack)  # (gapped positions may pass the LDS limit)
        same(dev_rates(gpu, fq, oq, pq, ft, ot, pt, pairs, RH.DEFAULT_RATES, 31, slack, scratch_bins=big), want)


@pytest.fixture(scope="module")
def scratch_case():
    """A 300-frame clip at 5/4 of a 1200-frame source, beside the LDS pairs of `planted`: under the default list the pair's
    largest histogram has 4 * 299 + 5 * 1199 + 1 + 10 = 7202 bins ((4, 5); the planted (5, 4) has 6302)."""
    rng = np.random.default_rng(63)
    source, clips = RH.planted_clips(seed=74, max_flips=20)
    L = rand(rng, 1200)
    clip = AH.noisy(rng, RH.resampled(L, 300, 5, 4, 17.4), 20)
    frames, offsets = RH.join([source, clips[(5, 4)], clips[(3, 2)], L, clip])
    pairs = [(1, 0), (4, 3), (0, 2), (3, 4), (2, 0), (4, 4), (1, 2)]
    return frames, offsets, pairs, RH.align_rates(frames, offsets, pairs)


def test_scratch_form_beside_lds_pairs(gpu, hvd, scratch_case):
    frames, offsets, pairs, want = scratch_case
    bins = bins_of(299, 1199, RH.DEFAULT_RATES, 1)
    assert bins == 7202 > LDS_BINS and bins_of(1199, 299, RH.DEFAULT_RATES, 1) == 7202
    assert want[1].tolist()[4:8] == (68, 300, 300, 300) and want[1].tolist()[12:15] == (5, 4, 1)  # 4 * 17.4 = 69.6, +- 2
    assert want[3]["offset"] == -68 and want[3].tolist()[12:15] == (4, 5, 2)
    same(hvd.search.align_rates(frames, offsets, pairs), want)
    same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES, scratch_bins=bins), want)
    # both launches write their own records and skip the other's: without scratch the scratch launch's pairs are lost, the
    # LDS launch's are intact
    lost = want.copy()
    for k in (1, 3):
        lost[k] = tuple(want[k].tolist()[:2]) + RH.LOST
    same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES, scratch_bins=0), lost)
    assert bins_of(299, 299, RH.DEFAULT_RATES, 1) <= LDS_BINS  # (the clip against itself is an LDS pair: 9 * 299 + 11 bins)


def test_a_pair_goes_to_the_scratch_launch_whole(gpu, hvd):
    """400 x 700 frames: 1101 bins at (1, 1), 4 * 399 + 5 * 699 + 1 + 10 = 5102 at (4, 5). Under [(1, 1), (4, 5)] the pair is the
    scratch launch's for both rounds: with scratch the restatement's record, without it the INT32_MIN record -- and under
    [(1, 1)] alone it needs none."""
    rng = np.random.default_rng(64)
    L = rand(rng, 700)
    A = AH.noisy(rng, L[150:550], 20)       # a 1x excerpt ...
    A[300:] = rand(rng, 100)                # ... of 300 frames
    frames, offsets = RH.join([A, L])
    rates = ((1, 1), (4, 5))
    assert bins_of(399, 699, rates[:1], 1) == 1101 and bins_of(399, 699, rates, 1) == 5102
    want = RH.align_rates(frames, offsets, [(0, 1), (1, 0)], None, rates)
    assert want[0].tolist()[4:8] == (150, 300, 300, 300) and want[0].tolist()[12:15] == (1, 1, 0)
    same(hvd.search.align_rates(frames, offsets, [(0, 1), (1, 0)], rates=rates), want)
    same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, [(0, 1), (1, 0)], rates, scratch_bins=5102), want)
    got = dev_rates(gpu, frames, offsets, None, frames, offsets, None, [(0, 1), (1, 0)], rates, scratch_bins=0)
    assert got.tolist() == [(0, 1) + RH.LOST, (1, 0) + RH.LOST]
    one = dev_rates(gpu, frames, offsets, None, frames, offsets, None, [(0, 1), (1, 0)], rates[:1], scratch_bins=0)
    same(one, RH.align_rates(frames, offsets, [(0, 1), (1, 0)], None, rates[:1]))


def test_scratch_one_word_too_small(gpu, hvd, scratch_case):
    """A slot holds the pair's largest histogram and its flag words: 7202 + ceil(300 / 32) + ceil(1200 / 32) = 7250 words. Told
    of exactly 64 such slots the entry aligns the pair; told of one word less per slot it gives the INT32_MIN record."""
    frames, offsets, pairs, want = scratch_case
    need = 7202 + 10 + 38
    args = (gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES)
    same(dev_rates(*args, scratch_bins=7202, scratch_bytes=4 * SLOTS * need), want)
    lost = want.copy()
    for k in (1, 3):
        lost[k] = tuple(want[k].tolist()[:2]) + RH.LOST
    same(dev_rates(*args, scratch_bins=7202, scratch_bytes=4 * SLOTS * need - 16), lost)


def test_broken_lists(gpu, hvd, planted):
    """The device entry: every pair gets the INT32_MIN record. The host entry: HVD_ERR_ARG."""
    frames, offsets, pairs, _, _ = planted
    for bad in (RH.NINE_RATES, [(2, 4)], [(1, 1), (1, 1)], [(0, 1)], [(1, 9)]):
        got = dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs[:3] + [(0, 9)], bad)
        assert got.tolist() == [tuple(p) + RH.LOST for p in pairs[:3] + [(0, 9)]], bad
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_rates(frames, offsets, pairs, rates=bad)
        assert e.value.code == gpu.HVD_ERR_ARG
    with pytest.raises(gpu.HvdError) as e:
        hvd.search.align_rates(frames, offsets, [(0, 9)])
    assert e.value.code == gpu.HVD_ERR_ARG


def test_many_small_pairs_grid_stride(gpu, hvd):
    """8 200 pairs of 4 x 4 frames, more than the 8 192 workgroups of the LDS launch: the first workgroups serve a second pair.
    Among them pair indices out of range (INT32_MIN), empty videos (the zero record) and pairs without a hit."""
    rng = np.random.default_rng(65)
    base = [rand(rng, 8) for _ in range(12)]
    vids = []
    for S in base:  # four 4-frame videos of one 8-frame source: 1x, 2x, 1x shifted, 1/2x
        vids += [S[0:4].copy(), S[[0, 2, 4, 6]].copy(), S[2:6].copy(), S[[1, 1, 2, 2]].copy()]
    vids += [np.zeros((0, 32), np.uint8), rand(rng, 4)]
    frames, offsets = RH.join(vids)
    V = len(vids)
    pairs = rng.integers(0, V, (LDS_GRID + 8, 2))
    pairs[rng.integers(0, len(pairs), 40), rng.integers(0, 2, 40)] = V + rng.integers(0, 3, 40)  # out of range
    pairs[[0, LDS_GRID - 1, LDS_GRID, LDS_GRID + 7]] = [(0, 1), (3, 0), (1, 0), (V, 0)]      # the first and the second round
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    want = RH.align_rates(frames, offsets, uniq)[inv.reshape(-1)]
    assert (want["offset"] == RH.INT32_MIN).sum() >= 30 and (want["q_hits"] == 0).sum() > 4000 and (want["q_hits"] > 0).sum() > 300
    same(dev_rates(gpu, frames, offsets, None, frames, offsets, None, pairs, RH.DEFAULT_RATES), want)


def test_find_rate_excerpts_end_to_end(gpu, hvd):
    """A 40-video library of frames in HBM with planted 1x, 5/4 and 2/3 excerpts. find_rate_excerpts reports all three,
    find_excerpts the 1x one alone; host entry, chained pipeline (positions from the quality filter through
    k_kept_positions: dropped frames leave gaps) and the rule on the restatement agree; with rates = ((1, 1),) the rate search
    IS the excerpt search."""
    S = hvd.synth
    longs = [S.frames_gray(150, seed=31, const_fraction=0.0), S.frames_gray(120, seed=32, const_fraction=0.0)]
    longs[0][[3, 40, 41, 77]] = 77  # constant frames: quality 0, dropped by the filter
    idx = lambda n, num, den, c: np.floor(np.arange(n) * num / den + c + 0.5).astype(np.int64)  # noqa: E731
    vids = [longs[0], longs[0][30:70].copy(), longs[0][idx(40, 5, 4, 20.3)].copy(), longs[1], longs[1][idx(45, 2, 3, 60.6)].copy()]
    vids += [S.frames_gray(12, seed=100 + k, const_fraction=0.0) for k in range(35)]
    assert len(vids) == 40
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    assert not keep[[3, 40, 41, 77]].any()
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(40)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(40)]
    positions = [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(40)]
    want = hvd.search.rate_excerpt_pairs(blobs, positions=positions, matcher=RH.ReferenceMatcher)
    by = {(e.short, e.long): e for e in want}
    assert by[(1, 0)].rate == 1 and by[(1, 0)].offset == 30
    assert by[(2, 0)].rate == Fraction(5, 4) and abs(by[(2, 0)].offset - Fraction(203, 10)) <= 1
    assert by[(4, 3)].rate == Fraction(2, 3) and abs(by[(4, 3)].offset - Fraction(606, 10)) <= 1
    assert all(by[p].coverage >= 90.0 for p in ((1, 0), (2, 0), (4, 3)))
    assert hvd.find_rate_excerpts(blobs, positions=positions) == want
    plain = hvd.find_excerpts(blobs, positions=positions)
    assert (1, 0) in [(e.short, e.long) for e in plain]
    assert not {(2, 0), (4, 3)} & {(e.short, e.long) for e in plain}
    one = hvd.find_rate_excerpts(blobs, rates=((1, 1),), positions=positions)
    assert [(e.short, e.long, e.offset, e.first, e.last, e.coverage, e.similarity) for e in one] == [tuple(e) for e in plain]
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        got, recs, aligned, library = hvd.pipeline.find_rate_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, keep_library=True)
        assert got == want
        assert np.array_equal(library.positions(), raw_pos) and np.array_equal(library.offsets(), kept_off)
        library.free()
        same(aligned, RH.align_rates(hashes[keep], kept_off, np.stack([recs["a"], recs["b"]], axis=1), raw_pos))
        single, _, _, _ = hvd.pipeline.find_rate_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, rates=((1, 1),))
        chained, _, _, _ = hvd.pipeline.find_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1)
        assert [(e.short, e.long, e.offset, e.first, e.last, e.coverage, e.similarity) for e in single] == [tuple(e) for e in chained]
        assert chained == plain
    finally:
        d_fr.free()
