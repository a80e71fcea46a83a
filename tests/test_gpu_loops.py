"""Looped clips and boomerangs on the GPU (run with -m gpu on an MI355X): k_valign_loops against the numpy
restatement of the rule (tests/loops_helpers.py) -- record for record, through the host entry, the device entry, Vpdq.align_loops,
DeviceLibrary.align_loops and the chained pipeline. Every comparison is equality. Record and scratch buffers of the device entry
end in sentinel tails that must stay intact."""
import ctypes as C

import numpy as np
import pytest

import align_helpers as AH
import loops_helpers as LH
import rates_helpers as RH
import signed_helpers as SG
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact
from test_gpu_signed import LDS_BINS, LDS_GRID, SLOTS

pytestmark = pytest.mark.gpu

REC = 416  # bytes of a record
RATES = LH.REVERSED_RATES
HEAD = ("a", "b", "q_hits", "t_hits", "n_segments", "q_covered", "t_covered", "rounds")


def dev_call(gpu, frames, offsets, positions, pairs, rates=RATES, max_dist=31, slack=1, max_rounds=64, min_band_votes=1,
             scratch_bins=0, entry="hvd_dev_vpdq_align_loops", dtype=LH.VLOOPS_DTYPE, scratch_entry="hvd_loops_scratch_bytes"):
    """The device entry with its own buffers, one library on both sides: records and scratch end in sentinel tails that must
    stay intact. -> (return code, records)."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    rates = np.ascontiguousarray(np.asarray(rates, dtype=np.int32).reshape(-1, 2))
    M = pairs.shape[0]
    sb = C.c_size_t(0)
    gpu.check(getattr(lib, scratch_entry)(scratch_bins, C.byref(sb)))
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(f=up(frames), o=up(np.asarray(offsets, np.int64)), p=up(None if positions is None else np.asarray(positions, np.int32)),
                pairs=up(pairs), out=_sentinel_buffer(gpu, REC * M), scr=_sentinel_buffer(gpu, sb.value) if sb.value else None)
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    V = len(offsets) - 1
    try:
        rc = getattr(lib, entry)(ptr("f"), ptr("o"), V, ptr("p"), ptr("f"), ptr("o"), V, ptr("p"), ptr("pairs"), M, max_dist, slack,
                                 rates.ctypes.data, rates.shape[0], max_rounds, min_band_votes, ptr("scr"), sb.value, ptr("out"))
        gpu.check(lib.hvd_dev_sync())
        out = bufs["out"].to_array(dtype, M)
        assert _tail_intact(gpu, bufs["out"], REC * M), "record buffer overrun"
        assert bufs["scr"] is None or _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return rc, out


def dev(gpu, frames, offsets, positions, pairs, **kwargs):
    rc, out = dev_call(gpu, frames, offsets, positions, pairs, **kwargs)
    gpu.check(rc)
    return out


@pytest.fixture(scope="module")
def planted():
    """video 0 a 120-frame source; 1 a boomerang of 12 + 12 frames; 2 a 3 x 10 loop; 3 ten repetitions of 6 frames; 4 a plain
    excerpt; 5 a reversed clip; 6, 7 a static pair; 8 random; 9 empty."""
    vids, pairs = LH.planted_loops(95)
    frames, offsets = RH.join(vids)
    return vids, frames, offsets, pairs


# ---- 1. a frame of b in two rounds ----

def test_boomerang_and_threefold_loop(gpu, hvd, planted):
    vids, _, _, _ = planted
    source40 = vids[0][20:60]  # holds the boomerang's 30..41 and the loop's 50..59
    frames, offsets = RH.join([vids[1], vids[2], source40])
    pairs = [(0, 2), (1, 2), (2, 0), (2, 1)]
    assert LH.shared_b_frames(vids[1], source40) > 0 and LH.shared_b_frames(vids[2], source40) > 0
    for floor in (1, 4):
        want = LH.align_loops(frames, offsets, pairs, min_band_votes=floor)
        if floor == 4:
            assert want[0].tolist()[4:8] == (2, 24, 12, 2) and sorted(want[0]["seg"][:2]["rate_num"].tolist()) == [-1, 1]
            assert want[1].tolist()[4:8] == (3, 30, 10, 3) and want[1]["seg"][:3]["t_aligned"].sum() == 30  # t_covered is distinct
            assert want[2]["rounds"] == 1  # the source as a: one round
        LH.same(hvd.search.align_loops(frames, offsets, pairs, min_band_votes=floor), want)
        LH.same(dev(gpu, frames, offsets, None, pairs, min_band_votes=floor), want)
    for (a, b), w in zip(pairs[:2], LH.align_loops(frames, offsets, pairs[:2])):
        rec = hvd.Vpdq.align_loops(frames[offsets[a]:offsets[a + 1]].tobytes(), hvd.VpdqHash(frames[offsets[b]:offsets[b + 1]].tobytes()))
        assert [int(rec[n]) for n in HEAD] == [0, 1] + [int(w[n]) for n in HEAD[2:]] and (rec["seg"] == w["seg"]).all()


# ---- 2. rounds past the eighth ----

@pytest.mark.parametrize("max_rounds", [8, 9, 64])
def test_rounds_past_the_eighth_write_no_segment(gpu, hvd, planted, max_rounds):
    """Ten repetitions of six frames: the ninth and tenth round add to rounds, q_covered and t_covered only, and the record of
    the NEXT pair in the list is intact."""
    _, frames, offsets, _ = planted
    pairs = [(3, 0), (4, 0), (3, 0), (1, 0)]
    want = LH.align_loops(frames, offsets, pairs, max_rounds=max_rounds, min_band_votes=4)
    n = min(max_rounds, 10)
    assert want[0].tolist()[4:8] == (8, 6 * n, 6, n) and want[1].tolist()[4:8] == (1, 20, 20, 1)
    assert want[0]["seg"]["q_aligned"].tolist() == [6] * 8
    LH.same(dev(gpu, frames, offsets, None, pairs, max_rounds=max_rounds, min_band_votes=4), want)
    LH.same(hvd.search.align_loops(frames, offsets, pairs, max_rounds=max_rounds, min_band_votes=4), want)


# ---- 3. the word edges of the three runs ----

def test_word_edges(gpu, hvd):
    """na and nb in {31, 32, 33, 64, 65}: the last frame of a run of bit words sits in the last bit of a word, in the first of the
    next, one further. Video a repeats seven frames of b, so every pair makes several rounds over the same frames of b."""
    rng = np.random.default_rng(96)
    S = RH._rand(rng, 65)
    sizes = (31, 32, 33, 64, 65)
    loops = [AH.noisy(rng, np.tile(S[20:27], (10, 1))[:n], 20) for n in sizes]
    frames, offsets = RH.join(loops + [S[:n].copy() for n in sizes])
    pairs = [(a, 5 + b) for a in range(5) for b in range(5)] + [(5 + b, a) for a in range(5) for b in range(5)]
    want = LH.align_loops(frames, offsets, pairs, min_band_votes=2)
    # (64 = 9 x 7 + 1: the one frame left over is a band of one hit, below the floor of two)
    assert want[:25]["rounds"].min() >= 5 and (want[:25]["q_covered"] == np.repeat((31, 32, 33, 63, 65), 5)).all()
    assert (want[:25]["t_covered"] == 7).all() and (want[:25]["rounds"] > 8).any() and (want[25:]["rounds"] == 1).all()
    LH.same(dev(gpu, frames, offsets, None, pairs, min_band_votes=2), want)
    LH.same(hvd.search.align_loops(frames, offsets, pairs, min_band_votes=2), want)


# ---- 4. past the stage chunk, on either side ----

def test_loop_and_source_past_256_frames(gpu, hvd):
    rng = np.random.default_rng(97)
    S = RH._rand(rng, 300)
    clip = S[120:180]
    vids = [AH.noisy(rng, np.tile(clip, (5, 1)), 20), clip.copy(),                                # a of 300 = 5 x 60 against b of 60
            AH.noisy(rng, np.concatenate([S[250:262], S[250:262][::-1]]), 20), S]                 # a short boomerang against b of 300
    frames, offsets = RH.join(vids)
    pairs = [(0, 1), (2, 3), (3, 2), (1, 0), (0, 3)]
    want = LH.align_loops(frames, offsets, pairs, min_band_votes=4)
    assert want[0].tolist()[4:8] == (5, 300, 60, 5) and want[1].tolist()[4:8] == (2, 24, 12, 2)
    assert want[4].tolist()[4:8] == (5, 300, 60, 5)
    assert max(SG.bins_of(299, 299, RATES, 1), SG.bins_of(299, 59, RATES, 1)) <= LDS_BINS
    LH.same(dev(gpu, frames, offsets, None, pairs, min_band_votes=4), want)
    LH.same(hvd.search.align_loops(frames, offsets, pairs, min_band_votes=4), want)


# ---- 5. the scratch form ----

@pytest.fixture(scope="module")
def stretched(planted):
    """The 3 x 10 loop (video 0), the boomerang (1) and the plain excerpt (2) against the source (3), whose last frame is moved
    out until the widest pair's largest bins_r is just above the LDS form's: 29 + 4065 + 1 + 2 = 4097."""
    vids, _, _, _ = planted
    frames, offsets = RH.join([vids[2], vids[1], vids[4], vids[0]])
    positions = np.concatenate([np.arange(30), np.arange(24), np.arange(20), np.arange(120)]).astype(np.int32)
    positions[-1] = 4065
    return frames, offsets, positions


def test_scratch_form_just_above_the_lds_bins(gpu, hvd, stretched):
    frames, offsets, positions = stretched
    bins = SG.bins_of(29, 4065, RATES, 1)
    assert bins == LDS_BINS + 1 and SG.bins_of(23, 4065, RATES, 1) <= LDS_BINS  # the boomerang's pair stays in LDS
    pairs = [(0, 3), (3, 0), (1, 3), (2, 3)]
    want = LH.align_loops(frames, offsets, pairs, positions, min_band_votes=4)
    assert want[0].tolist()[4:8] == (3, 30, 10, 3) and want[1]["rounds"] == 1 and want[2].tolist()[4:8] == (2, 24, 12, 2)
    LH.same(dev(gpu, frames, offsets, positions, pairs, min_band_votes=4, scratch_bins=bins), want)
    LH.same(hvd.search.align_loops(frames, offsets, pairs, positions, min_band_votes=4), want)
    gone = want.copy()  # without scratch the two big pairs are lost, the LDS ones stay
    gone[0], gone[1] = LH.lost_record(0, 3), LH.lost_record(3, 0)
    LH.same(dev(gpu, frames, offsets, positions, pairs, min_band_votes=4, scratch_bins=0), gone)


def test_bin_limit_at_minus_eight(gpu, hvd):
    """(-8, 1) at slack 1: 8 span_a + span_b + 1 + 16 = 2^20 bins align, one more gives the INT32_MIN record."""
    rng = np.random.default_rng(92)
    A = RH._rand(rng, 2)
    frames, offsets = RH.join([A, AH.noisy(rng, A, 20), AH.noisy(rng, A, 20)])
    positions = np.array([0, 131069, 0, 7, 0, 8], dtype=np.int32)
    assert SG.bins_of(131069, 7, ((-8, 1),), 1) == 1 << 20
    pairs = [(0, 1), (0, 2)]
    want = LH.align_loops(frames, offsets, pairs, positions, ((-8, 1),))
    assert want[0]["rounds"] == 2 and sorted(want[0]["seg"][:2]["offset"].tolist()) == [0, 8 * 131069 + 7]
    assert want[1] == LH.lost_record(0, 2)
    LH.same(dev(gpu, frames, offsets, positions, pairs, rates=((-8, 1),), scratch_bins=1 << 20), want)


def test_slots_serve_several_pairs(gpu, hvd, stretched):
    """130 pairs of the scratch form over 64 slots: a slot's second and third pair find the taken and the seen words of the one
    before, which must have been cleared -- the pair that follows a loop in a slot is another one."""
    frames, offsets, positions = stretched
    positions = positions.copy()
    positions[-1] = 4075  # ten more: the boomerang's and the plain excerpt's pair need the scratch as well
    three = [(0, 3), (2, 3), (1, 3)]
    assert all(SG.bins_of(span, 4075, RATES, 1) > LDS_BINS for span in (29, 19, 23))
    pairs = [three[k % 3] for k in range(130)]
    assert pairs[0] != pairs[SLOTS] != pairs[2 * SLOTS]
    want = LH.restated(frames, offsets, pairs, positions, RATES, 64, 4)
    assert want[0]["rounds"] == 3 and want[1]["rounds"] == 1 and want[2]["rounds"] == 2
    LH.same(dev(gpu, frames, offsets, positions, pairs, min_band_votes=4, scratch_bins=4200), want)


# ---- 6. more pairs than workgroups ----

def test_more_pairs_than_workgroups(gpu, hvd, planted):
    """8192 + 300 small pairs drawn from the planted ones: the first workgroups serve a second pair where the first one's taken
    and seen words still lie in LDS. The restatement is computed once per distinct pair."""
    _, frames, offsets, distinct = planted
    rng = np.random.default_rng(98)
    order = rng.integers(0, len(distinct), LDS_GRID + 300)
    order[[0, LDS_GRID]] = [2, 3]      # workgroup 0: the ten-fold loop, then the plain excerpt
    order[[1, LDS_GRID + 1]] = [0, 13]  # workgroup 1: the boomerang, then an empty video
    pairs = [distinct[k] for k in order]
    assert pairs[0] == (3, 0) and pairs[LDS_GRID] == (4, 0) and pairs[LDS_GRID + 1] == (9, 0)
    want = LH.restated(frames, offsets, pairs, None, RATES, 64, 2)
    assert want[0]["rounds"] == 10 and want[LDS_GRID]["rounds"] == 1 and want[LDS_GRID + 1]["q_hits"] == 0
    LH.same(dev(gpu, frames, offsets, None, pairs, min_band_votes=2), want)


# ---- 7. consequence (1) on the device ----

def test_first_segment_is_the_signed_entrys(gpu, hvd, planted):
    _, frames, offsets, pairs = planted
    for rates, floor in ((RATES, 1), (SG.FOUR_RATES, 4), (((-1, 1), (1, 1)), 1)):
        got = dev(gpu, frames, offsets, None, pairs, rates=rates, min_band_votes=floor)
        sgn = dev(gpu, frames, offsets, None, pairs, rates=rates, max_rounds=8, min_band_votes=floor, entry="hvd_dev_vpdq_align_signed",
                  dtype=SG.VSSEGMENTS_DTYPE, scratch_entry="hvd_signed_scratch_bytes")
        assert np.array_equal(np.ascontiguousarray(got["seg"][:, 0]).view(np.uint32), np.ascontiguousarray(sgn["seg"][:, 0]).view(np.uint32))
        assert np.array_equal(got["q_hits"], sgn["q_hits"]) and np.array_equal(got["t_hits"], sgn["t_hits"])
        assert (got["rounds"] > sgn["n_segments"]).any()
        one = dev(gpu, frames, offsets, None, pairs, rates=rates, max_rounds=1, min_band_votes=floor)  # consequence (4)
        sg1 = dev(gpu, frames, offsets, None, pairs, rates=rates, max_rounds=1, min_band_votes=floor, entry="hvd_dev_vpdq_align_signed",
                  dtype=SG.VSSEGMENTS_DTYPE, scratch_entry="hvd_signed_scratch_bytes")
        assert np.array_equal(one["rounds"], one["n_segments"])
        one["rounds"] = 0
        assert np.array_equal(one.view(np.uint32), sg1.view(np.uint32))


# ---- 8. bad pairs, broken lists ----

def test_pair_out_of_range_empty_video_and_broken_lists(gpu, hvd, planted):
    _, frames, offsets, _ = planted
    pairs = [(10, 0), (1, 0), (0, 10), (9, 0), (0, 9), (9, 9), (3, 0)]
    want = LH.align_loops(frames, offsets, pairs)
    assert want[0] == LH.lost_record(10, 0) and want[2] == LH.lost_record(0, 10)
    assert want[3].tolist()[2:8] == (0,) * 6 and want[3]["seg"][0]["offset"] == 0  # an empty video: the zero record
    LH.same(dev(gpu, frames, offsets, None, pairs), want)
    with pytest.raises(gpu.HvdError) as e:
        hvd.search.align_loops(frames, offsets, pairs[:2])
    assert e.value.code == gpu.HVD_ERR_ARG
    LH.same(hvd.search.align_loops(frames, offsets, pairs[3:]), want[3:])
    some = [(1, 0), (0, 1), (0, 12)]
    for bad in SG.BROKEN_LISTS[:-1]:
        LH.same(dev(gpu, frames, offsets, None, some, rates=bad), np.array([LH.lost_record(*p) for p in some], dtype=LH.VLOOPS_DTYPE))
    for k in (0, 65):
        rc, _ = dev_call(gpu, frames, offsets, None, some[:2], max_rounds=k)
        assert rc == gpu.HVD_ERR_ARG


# ---- 9. library and pipeline ----

def test_library_and_pipeline(gpu, hvd):
    """A small library of frames in HBM with a boomerang, a four-fold loop and a plain excerpt planted ahead of their sources.
    DeviceLibrary.align_loops equals search.align_loops; the chained pipeline, the host search and the rule on the restatement
    agree and find all three, the loops at more than one round; the signed search covers the loops by one repetition."""
    S = hvd.synth
    longs = [S.frames_gray(200, seed=61, const_fraction=0.0), S.frames_gray(160, seed=62, const_fraction=0.0)]
    longs[0][[3, 140]] = 77  # constant frames: quality 0, dropped by the filter
    half = longs[0][100:130]
    vids = [np.concatenate([half, half[::-1]]), longs[0], np.tile(longs[1][50:65], (4, 1, 1)), longs[1], longs[1][20:60].copy()]
    vids += [S.frames_gray(12, seed=400 + k, const_fraction=0.0) for k in range(6)]
    V = len(vids)
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(V)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(V)]
    positions = [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(V)]
    want = hvd.search.looped_excerpt_pairs(blobs, positions=positions, matcher=LH.ReferenceMatcher)
    by = {(e.loop, e.source): e for e in want}
    assert by[0, 1].coverage == 100.0 and by[0, 1].rounds == 2 and sorted(s.rate for s in by[0, 1].segments) == [-1, 1]
    assert by[2, 3].coverage == 100.0 and by[2, 3].rounds == 4 and by[2, 3].source_frames == len(positions[2]) // 4 >= 12  # (the filter dropped some of the 15)
    assert by[4, 3].coverage == 100.0 and by[4, 3].rounds == 1
    assert hvd.find_looped_excerpts(blobs, positions=positions) == want
    today = {(e.short, e.long): int(e.coverage) for e in hvd.find_reversed_excerpts(blobs, positions=positions)}
    assert today.get((0, 1), 0) <= 52 and (2, 3) not in today
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        chained, recs, aligned, library = hvd.pipeline.find_looped_excerpts_on_device(d_fr.ptr, raw_off, 64, 64, 1, keep_library=True)
        try:
            assert chained == want
            ab = np.stack([recs["a"], recs["b"]], axis=1)
            both = np.concatenate([ab, ab[:, ::-1]])
            LH.same(aligned, LH.align_loops(hashes[keep], kept_off, both, raw_pos, min_band_votes=4))
            for rates, rounds in ((RATES, 64), (SG.FOUR_RATES, 3)):
                LH.same(library.align_loops(both, rates=rates, max_rounds=rounds),
                        hvd.search.align_loops(hashes[keep], kept_off, both, raw_pos, rates=rates, max_rounds=rounds))
        finally:
            library.free()
    finally:
        d_fr.free()


# ---- 10. the table of the proposal through the host entry, the device entry and the search ----

@pytest.fixture(scope="module")
def table_library():
    """videos 0..5 = source, boom, loop5, loop12, boom3, clip of loops_helpers.table(); 6, 7 = the static 50 / 80 pair. Every
    loop against the source in both orientations, the static pair both ways."""
    t = LH.table()
    A, B = LH.static_pair()
    frames, offsets = RH.join([t["source"], t["boom"], t["loop5"], t["loop12"], t["boom3"], t["clip"], A, B])
    pairs = [(v, 0) for v in range(1, 6)] + [(0, v) for v in range(1, 6)] + [(6, 7), (7, 6)]
    assert max(SG.bins_of(599, 299, RATES, 1), SG.bins_of(299, 599, RATES, 1)) <= LDS_BINS  # the LDS form
    return frames, offsets, pairs


@pytest.mark.parametrize("max_rounds", [8, 64])
def test_table_in_both_orientations(gpu, hvd, table_library, max_rounds):
    """Every line of the table, a = the loop and a = the source, at floor 4: the host entry and the device entry give the
    restatement's records, whose figures are the table's."""
    frames, offsets, pairs = table_library
    want = LH.align_loops(frames, offsets, pairs, max_rounds=max_rounds, min_band_votes=4)
    figures = [tuple(int(w[n]) for n in ("rounds", "q_covered", "t_covered")) for w in want]
    twelve = (12, 240, 20) if max_rounds == 64 else (8, 160, 20)
    assert figures[:5] == [(2, 120, 60), (5, 300, 60), twelve, (6, 180, 30), (1, 60, 60)]
    assert [(int(s["rate_num"]), int(s["offset"]), int(s["q_aligned"])) for s in want[0]["seg"][:2]] == [(1, 100, 61), (-1, 219, 59)]
    assert want[1]["seg"][:5]["offset"].tolist() == [-20, 40, -80, 100, -140] and want[2]["n_segments"] == 8
    assert sorted(want[3]["seg"][:6]["rate_num"].tolist()) == [-1, -1, -1, 1, 1, 1]
    assert all(f[0] == 1 for f in figures[5:10])  # the source as a: one round, one repetition's frames
    assert want[10]["seg"][0].tolist() == (1, 150, 50, 52, 0, 49, 0, 51, 1, 1, 0, 0) and figures[10] == (1, 50, 52)
    for got in (hvd.search.align_loops(frames, offsets, pairs, max_rounds=max_rounds, min_band_votes=4),
                dev(gpu, frames, offsets, None, pairs, max_rounds=max_rounds, min_band_votes=4)):
        LH.same(got, want)
        # consequences (2) and (3) on the kernel's own words
        for g in got:
            votes = g["seg"]["band_votes"][:int(g["n_segments"])].tolist()
            assert votes == sorted(votes, reverse=True)
            if g["rounds"] <= 8:
                assert int(g["q_covered"]) == int(g["seg"]["q_aligned"].sum())
            else:
                assert int(g["q_covered"]) > int(g["seg"]["q_aligned"].sum()) and int(g["n_segments"]) == 8
            assert int(g["t_covered"]) <= int(g["t_hits"])
            if g["rounds"] <= 8:  # distinct frames of b: never more than the rounds' frames of b together
                assert int(g["t_covered"]) <= int(g["seg"]["t_aligned"].sum())


def test_find_looped_excerpts_reports_the_boomerang_and_the_twelve_fold_loop(gpu, hvd):
    """What no search reported before: the 60 + 60 boomerang and the twelve-fold loop of 20 frames come back from
    find_looped_excerpts -- video search and kernel -- at coverage 100, in 2 and in 12 rounds; at max_rounds 8 the loop is
    covered 8 / 12. The result is the fold's on the reference matcher."""
    t = LH.table()
    blobs = [v.tobytes() for v in (t["boom"], t["loop12"], t["source"], t["clip"])]
    got = hvd.find_looped_excerpts(blobs)
    assert got == hvd.search.looped_excerpt_pairs(blobs, matcher=LH.ReferenceMatcher)
    by = {(e.loop, e.source): e for e in got}
    assert sorted(by) == [(0, 2), (1, 2), (3, 2)]
    assert (by[0, 2].coverage, by[0, 2].rounds, by[0, 2].source_frames) == (100.0, 2, 60)
    assert (by[1, 2].coverage, by[1, 2].rounds, by[1, 2].source_frames, len(by[1, 2].segments)) == (100.0, 12, 20, 8)
    assert (by[3, 2].coverage, by[3, 2].rounds) == (100.0, 1)
    eight = {(e.loop, e.source): e for e in hvd.find_looped_excerpts(blobs, max_rounds=8)}
    assert int(eight[1, 2].coverage) == 66 and eight[1, 2].rounds == 8
    today = {(e.short, e.long): int(e.coverage) for e in hvd.find_reversed_excerpts(blobs)}
    assert today == {(0, 2): 50, (3, 2): 100}
