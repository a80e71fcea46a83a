"""Time alignment with negative rates on the GPU (run with -m gpu on an MI355X): k_valign_signed against the numpy
restatement of the rule (tests/signed_helpers.py) -- record for record and word for word, through the host entry, the device
entry, Vpdq.align_signed, DeviceLibrary.align_signed and the chained pipeline. Every comparison is equality. Record and scratch
buffers of the device entry end in sentinel tails that must stay intact."""
import ctypes as C

import numpy as np
import pytest

import align_helpers as AH
import rate_segments_helpers as RS
import rates_helpers as RH
import signed_helpers as SG
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

LDS_BINS = 4096   # HVD_ALIGN_LDS_BINS
LDS_GRID = 8192   # workgroups of the LDS launch at most (launch_lds_then_scratch)
SLOTS = 64        # workgroups of the scratch launch, one slot of the scratch each
REC = 416         # bytes of a record
HEAD = ("a", "b", "q_hits", "t_hits", "n_segments", "q_covered", "t_covered", "reserved")


def dev_call(gpu, fq, oq, pq, ft, ot, pt, pairs, rates, max_dist=31, slack=1, max_segments=8, min_band_votes=1, scratch_bins=0,
             scratch_bytes=None, entry="hvd_dev_vpdq_align_signed", dtype=SG.VSSEGMENTS_DTYPE):
    """The device entry with its own buffers: records and scratch end in sentinel tails that must stay intact. scratch_bytes:
    what the entry is TOLD it has (the buffer itself is sized for scratch_bins). -> (return code, records)."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    rates = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
    M = pairs.shape[0]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_signed_scratch_bytes(scratch_bins, C.byref(sb)))
    told = sb.value if scratch_bytes is None else scratch_bytes
    assert told <= sb.value
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(fq=up(fq), oq=up(np.asarray(oq, np.int64)), pq=up(None if pq is None else np.asarray(pq, np.int32)),
                ft=up(ft), ot=up(np.asarray(ot, np.int64)), pt=up(None if pt is None else np.asarray(pt, np.int32)),
                pairs=up(pairs), out=_sentinel_buffer(gpu, REC * M), scr=_sentinel_buffer(gpu, sb.value) if sb.value else None)
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    try:
        rc = getattr(lib, entry)(ptr("fq"), ptr("oq"), len(oq) - 1, ptr("pq"), ptr("ft"), ptr("ot"), len(ot) - 1, ptr("pt"),
                                 ptr("pairs"), M, max_dist, slack, rates.ctypes.data, rates.shape[0], max_segments,
                                 min_band_votes, ptr("scr"), told, ptr("out"))
        gpu.check(lib.hvd_dev_sync())
        out = bufs["out"].to_array(dtype, M)
        assert _tail_intact(gpu, bufs["out"], REC * M), "record buffer overrun"
        assert bufs["scr"] is None or _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return rc, out


def dev(gpu, frames, offsets, positions, pairs, rates, **kwargs):
    """One library on both sides."""
    rc, out = dev_call(gpu, frames, offsets, positions, frames, offsets, positions, pairs, rates, **kwargs)
    gpu.check(rc)
    return out


def lost(pairs):
    return np.array([SG.lost_record(*p) for p in pairs], dtype=SG.VSSEGMENTS_DTYPE)


# ---- 1. the table, LDS form ----

@pytest.mark.parametrize("listed", ["reversed", "four"])
def test_table_in_both_orientations(gpu, hvd, listed):
    frames, offsets, pairs = SG.table_library()
    rates = SG.REVERSED_RATES if listed == "reversed" else SG.FOUR_RATES
    assert max(SG.bins_of(599, 109, rates, 1), SG.bins_of(109, 599, rates, 1)) <= LDS_BINS  # the LDS form
    for floor in (1, 4):
        for K in (1, 3, 8):
            want = SG.align_signed(frames, offsets, pairs, None, rates, max_segments=K, min_band_votes=floor)
            if K == 8:  # the records of the proposal
                assert want[0]["seg"][0].tolist() == (159, 60, 60, 60, 0, 59, 100, 159, -1, 1, 1, 0)
                assert want[1]["seg"][0].tolist() == (159, 60, 60, 60, 100, 159, 0, 59, -1, 1, 1, 0)
            if K == 8 and floor == 4 and listed == "four":
                assert want[4].tolist()[4:7] == (3, 110, 110)
                assert [s.tolist()[8:11] for s in want[4]["seg"][:3]] == [(1, 1, 0), (-1, 1, 1), (-2, 1, 3)]
                assert want[4]["seg"][:3]["offset"].tolist() == [50, 479, 460]
            SG.same(hvd.search.align_signed(frames, offsets, pairs, rates=rates, max_segments=K, min_band_votes=floor), want)
            SG.same(dev(gpu, frames, offsets, None, pairs, rates, max_segments=K, min_band_votes=floor), want)
            if floor == 1:
                for (a, b), w in zip(pairs, want):
                    rec = hvd.Vpdq.align_signed(frames[offsets[a]:offsets[a + 1]].tobytes(),
                                                hvd.VpdqHash(frames[offsets[b]:offsets[b + 1]].tobytes()), rates=rates, max_segments=K)
                    assert [rec[n] for n in HEAD] == [0, 1] + [w[n] for n in HEAD[2:]] and (rec["seg"] == w["seg"]).all()
    want = SG.align_signed(frames, offsets, pairs[2:4], None, SG.LIST_32)  # (-3, 2) in the 8th place
    assert want[0]["seg"][0].tolist() == (600, 40, 40, 40, 0, 39, 242, 300, -3, 2, 7, 0)
    SG.same(dev(gpu, frames, offsets, None, pairs[2:4], SG.LIST_32), want)


# ---- 2. corner bins ----

def test_corner_bins(gpu, hvd):
    """Two hits, in the first and in the last core bin of the histogram at (-1, 1)."""
    rng = np.random.default_rng(77)
    a, b = RH._rand(rng, 30), RH._rand(rng, 50)
    a[0], a[29] = b[0], b[49]
    frames, offsets = RH.join([a, b])
    shifted = np.concatenate([np.arange(30) + 7, np.arange(50) + 11]).astype(np.int32)
    for positions, offs in ((None, [0, 78]), (shifted, [18, 96])):
        for pairs in ([(0, 1)], [(1, 0)]):
            want = SG.align_signed(frames, offsets, pairs, positions, ((-1, 1),), max_segments=2)
            assert want[0]["n_segments"] == 2 and want[0]["seg"][:2]["offset"].tolist() == offs
            assert want[0]["seg"][:2]["band_votes"].tolist() == [1, 1]
            SG.same(dev(gpu, frames, offsets, positions, pairs, ((-1, 1),), max_segments=2), want)
            SG.same(hvd.search.align_signed(frames, offsets, pairs, positions, ((-1, 1),), max_segments=2), want)


# ---- 3. the scratch form ----

@pytest.fixture(scope="module")
def long_source():
    """The reversed 60-frame clip (video 0) and a forward one (video 2) of a 4100-frame source (video 1): 4161 bins at (-1, 1)."""
    rng = np.random.default_rng(90)
    source = RH._rand(rng, 4100)
    frames, offsets = RH.join([AH.noisy(rng, source[3000:3060][::-1], 20), source, AH.noisy(rng, source[17:77], 20)])
    return frames, offsets


def test_scratch_form(gpu, hvd, long_source):
    frames, offsets = long_source
    bins = SG.bins_of(59, 4099, SG.REVERSED_RATES, 1)
    assert bins == 4161 > LDS_BINS
    pairs = [(0, 1), (1, 0), (2, 1), (0, 2)]
    want = SG.align_signed(frames, offsets, pairs)
    assert want[0]["seg"][0].tolist() == (3059, 60, 60, 60, 0, 59, 3000, 3059, -1, 1, 1, 0)
    assert want[1]["seg"][0].tolist() == (3059, 60, 60, 60, 3000, 3059, 0, 59, -1, 1, 1, 0)
    assert want[2]["seg"][0].tolist()[8:11] == (1, 1, 0) and want[3]["q_hits"] == 0
    SG.same(dev(gpu, frames, offsets, None, pairs, SG.REVERSED_RATES, scratch_bins=bins), want)
    SG.same(hvd.search.align_signed(frames, offsets, pairs), want)
    # too small a told scratch: a slot holds 4161 + 2 * (2 + 129) words; 16 bytes less and the big pairs are lost
    need = 4161 + 2 * (2 + 129)
    gone = want.copy()
    gone[:3] = lost(pairs[:3])
    SG.same(dev(gpu, frames, offsets, None, pairs, SG.REVERSED_RATES, scratch_bins=bins, scratch_bytes=4 * SLOTS * need), want)
    SG.same(dev(gpu, frames, offsets, None, pairs, SG.REVERSED_RATES, scratch_bins=bins, scratch_bytes=4 * SLOTS * need - 16), gone)
    SG.same(dev(gpu, frames, offsets, None, pairs, SG.REVERSED_RATES, scratch_bins=0), gone)


# ---- 4. top nibble and sign placement ----

@pytest.fixture(scope="module")
def planted():
    vids, pairs = SG.planted_signed(91)
    frames, offsets = RH.join(vids)
    return frames, offsets, pairs


@pytest.mark.parametrize("max_dist", [0, 31, 32])
def test_top_nibble_and_sign_placement(gpu, hvd, planted, max_dist):
    frames, offsets, pairs = planted
    turned = RH.rotated(SG.WIDE_SIGNED, 3)
    assert turned[0][0] < 0 and turned[-1][0] < 0 and SG.WIDE_SIGNED[0][0] > 0 and SG.WIDE_SIGNED[-1] == (-8, 1)
    for rates in (((-8, 1),), SG.WIDE_SIGNED, turned):
        assert SG.sound_signed(rates)
        for slack in (0, 1, 16):
            assert max(SG.bins_of(299, 35, rates, slack), SG.bins_of(35, 299, rates, slack)) <= LDS_BINS
            want = SG.restated(frames, offsets, pairs, None, rates, slack, max_dist)
            if max_dist == 31 and slack == 1 and len(rates) == 8:  # the planted rates are found, the reversed ones among them
                found = {tuple(w["seg"][0].tolist()[8:10]) for w in want[:8] if w["n_segments"]}
                assert {(-7, 8), (-8, 3), (-8, 1), (8, 7), (7, 2)} <= found, found
            SG.same(dev(gpu, frames, offsets, None, pairs, rates, max_dist=max_dist, slack=slack), want)
    SG.same(hvd.search.align_signed(frames, offsets, pairs, rates=turned, slack=16, max_dist=max_dist), want)


# ---- 5. the bin limit ----

def test_bin_limit_at_minus_eight(gpu, hvd):
    """(-8, 1) at slack 1: 8 span_a + span_b + 1 + 16 = 2^20 bins align, one more gives the INT32_MIN record. Two hits, in
    the first and in the last core bin."""
    rng = np.random.default_rng(92)
    A = RH._rand(rng, 2)
    frames, offsets = RH.join([A, AH.noisy(rng, A, 20), AH.noisy(rng, A, 20)])
    positions = np.array([0, 131069, 0, 7, 0, 8], dtype=np.int32)
    assert 8 * 131069 + 7 == (1 << 20) - 17 and SG.bins_of(131069, 7, ((-8, 1),), 1) == 1 << 20
    pairs = [(0, 1), (0, 2)]
    want = SG.align_signed(frames, offsets, pairs, positions, ((-8, 1),))
    assert want[0]["n_segments"] == 2 and sorted(want[0]["seg"][:2]["offset"].tolist()) == [0, 8 * 131069 + 7]
    assert want[1] == SG.lost_record(0, 2)
    SG.same(dev(gpu, frames, offsets, positions, pairs, ((-8, 1),), scratch_bins=1 << 20), want)


# ---- 6. many pairs ----

def test_many_pairs_share_workgroups_and_slots(gpu, hvd, long_source):
    """8192 + 300 small pairs drawn from a dozen distinct ones: the first workgroups serve a second pair, a reverse-winning one
    and then a forward-winning or an empty one. 70 big pairs: the workgroup of a slot serves two, the second where the first
    one's taken words still lie. The restatement is computed once per distinct pair."""
    big_frames, big_offsets = long_source
    rng = np.random.default_rng(93)
    S = RH._rand(rng, 40)
    small = [S[5:25][::-1].copy(), S, S[10:30].copy(), np.concatenate([S[0:10], S[30:40][::-1]]), RH._rand(rng, 6),
             np.zeros((0, 32), np.uint8)]
    frames, offsets = RH.join([big_frames[big_offsets[v]:big_offsets[v + 1]] for v in range(3)] + small)
    distinct = [(3, 4), (4, 3), (5, 4), (4, 5), (6, 4), (4, 6), (7, 4), (8, 4), (3, 5), (3, 6), (6, 3), (4, 4)]
    order = rng.integers(0, len(distinct), LDS_GRID + 300)
    order[[0, LDS_GRID]] = [0, 2]   # workgroup 0: a reverse-winning pair, then a forward-winning one
    order[[1, LDS_GRID + 1]] = [0, 7]  # workgroup 1: a reverse-winning pair, then an empty one
    pairs = [distinct[k] for k in order]
    bigs = [(0, 1), (1, 0), (2, 1)]
    pairs = [bigs[k % 3] for k in range(70)] + pairs
    assert pairs[0] != pairs[SLOTS]
    want = SG.restated(frames, offsets, pairs, None, SG.REVERSED_RATES, min_band_votes=2)
    first = {p: want[pairs.index(p)] for p in distinct}
    assert first[(3, 4)]["seg"][0]["rate_num"] == -1 and first[(5, 4)]["seg"][0]["rate_num"] == 1 and first[(8, 4)]["q_hits"] == 0
    assert first[(6, 4)]["n_segments"] == 2 and sorted(first[(6, 4)]["seg"][:2]["rate_num"].tolist()) == [-1, 1]
    SG.same(dev(gpu, frames, offsets, None, pairs, SG.REVERSED_RATES, min_band_votes=2, scratch_bins=4161), want)


# ---- 7. (a) on the device ----

def test_forward_lists_are_the_rate_segments_kernel(gpu, hvd, long_source):
    """An all-positive list against hvd_dev_vpdq_align_rate_segments on the same buffers, word for word; a broken list gives
    every pair the INT32_MIN record and the host entry HVD_ERR_ARG."""
    for source, reel in (RS.reel_b(), RS.reel_c()):
        frames, offsets = RH.join([reel, source])
        for K, floor in ((8, 1), (8, 4), (1, 1)):
            args = (gpu, frames, offsets, None, frames, offsets, None, [(0, 1), (1, 0)], RH.DEFAULT_RATES)
            rc, got = dev_call(*args, max_segments=K, min_band_votes=floor)
            rc2, fwd = dev_call(*args, max_segments=K, min_band_votes=floor, entry="hvd_dev_vpdq_align_rate_segments",
                                dtype=RS.VRSEGMENTS_DTYPE)
            assert rc == rc2 == 0
            SG.same_words(got, fwd)
            RS.same(fwd, RS.align_rate_segments(frames, offsets, [(0, 1), (1, 0)], max_segments=K, min_band_votes=floor))
    frames, offsets = long_source  # the scratch form
    args = (gpu, frames, offsets, None, frames, offsets, None, [(0, 1), (2, 1), (1, 2)], ((1, 1), (2, 1)))
    rc, got = dev_call(*args, scratch_bins=8300)
    rc2, fwd = dev_call(*args, scratch_bins=8300, entry="hvd_dev_vpdq_align_rate_segments", dtype=RS.VRSEGMENTS_DTYPE)
    assert rc == rc2 == 0 and fwd[1]["seg"][0]["q_aligned"] == 60
    SG.same_words(got, fwd)
    some = [(0, 1), (1, 0), (0, 9)]
    for bad in SG.BROKEN_LISTS[:-1]:
        SG.same(dev(gpu, frames, offsets, None, some, bad, scratch_bins=4161), lost(some))
        with pytest.raises(gpu.HvdError) as e:
            hvd.search.align_signed(frames, offsets, some[:2], rates=bad)
        assert e.value.code == gpu.HVD_ERR_ARG
    with pytest.raises(gpu.HvdError) as e:  # the existing entry keeps rejecting a negative num
        hvd.search.align_rate_segments(frames, offsets, some[:2], rates=SG.REVERSED_RATES)
    assert e.value.code == gpu.HVD_ERR_ARG


# ---- 8. library and pipeline ----

def test_library_and_pipeline(gpu, hvd):
    """A small library of frames in HBM with one reversed clip and one reel (forward, reversed, reversed at 2x) planted ahead
    of their sources. DeviceLibrary.align_signed equals search.align_signed; the chained pipeline, the host search and the rule
    on the restatement agree and find both; the forward search finds neither."""
    S = hvd.synth
    longs = [S.frames_gray(300, seed=51, const_fraction=0.0), S.frames_gray(260, seed=52, const_fraction=0.0)]
    longs[0][[3, 140]] = 77  # constant frames: quality 0, dropped by the filter
    back = lambda n, num, c: np.floor(c - np.arange(n) * num + 0.5).astype(np.int64)  # noqa: E731
    reel = np.concatenate([np.arange(20, 44), np.arange(200, 224)[::-1], back(20, 2, 139.6)])
    vids = [longs[0][100:160][::-1].copy(), longs[0], longs[1][reel].copy(), longs[1]]
    vids += [S.frames_gray(12, seed=300 + k, const_fraction=0.0) for k in range(12)]
    V = len(vids)
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(V)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(V)]
    positions = [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(V)]
    want = hvd.search.signed_excerpt_pairs(blobs, rates=SG.FOUR_RATES, positions=positions, matcher=SG.ReferenceMatcher)
    by = {(e.short, e.long): e for e in want}
    assert by[(0, 1)].coverage >= 90.0 and [s.rate for s in by[(0, 1)].segments] == [-1]
    assert by[(2, 3)].coverage >= 90.0 and [s.rate for s in by[(2, 3)].segments] == [1, -1, -2]
    assert hvd.find_reversed_excerpts(blobs, rates=SG.FOUR_RATES, positions=positions) == want
    forward = hvd.find_rate_segmented_excerpts(blobs, positions=positions)
    assert not {(0, 1), (2, 3)} & {(e.short, e.long) for e in forward}
    positive = ((1, 1), (2, 1))
    assert hvd.find_reversed_excerpts(blobs, rates=positive, positions=positions) == \
        hvd.find_rate_segmented_excerpts(blobs, rates=positive, positions=positions)
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        chained, recs, aligned, library = hvd.pipeline.find_reversed_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1,
                                                                                        rates=SG.FOUR_RATES, keep_library=True)
        try:
            assert chained == want
            pairs = np.stack([recs["a"], recs["b"]], axis=1)
            SG.same(aligned, SG.align_signed(hashes[keep], kept_off, pairs, raw_pos, SG.FOUR_RATES, min_band_votes=4))
            for rates, K in ((SG.REVERSED_RATES, 8), (SG.FOUR_RATES, 2)):
                SG.same(library.align_signed(recs, rates=rates, max_segments=K),
                        hvd.search.align_signed(hashes[keep], kept_off, pairs, raw_pos, rates=rates, max_segments=K))
        finally:
            library.free()
    finally:
        d_fr.free()
