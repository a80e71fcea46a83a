"""The duration-weighted search end to end on the GPU, on the planted library of tests/runs_helpers.py collapsed at
PLANTED_MAX_DIST with weights = run. Uncapped, a kept frame counts for its whole hold: the six copies AND (C, D), at 60 of 100,
as on the raw library. Capped at 9 -- no hold of a copy is longer -- the six copies alone: C-D is 9 of 49. Capped at 1: the plain
search of the collapsed library. Pairs, records and groups are the model's (tests/weighted_helpers.py), through the host entries
and through the chained device pipeline; tests/test_weighted_cpu.py checks the same figures by the model alone."""
import numpy as np
import pytest

import runs_helpers as RH
import weighted_helpers as WH

pytestmark = pytest.mark.gpu

CAPS = (0, 9, 1)


def _T(hvd):
    return hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)


def _model(hvd, frames, offsets):
    """The collapse and, per cap, (rows, totals, pairs at threshold 50) by the model."""
    keep, run = RH.model_runs(frames, offsets, RH.PLANTED_MAX_DIST)
    f2, o2, _, dropped = RH.model_collapsed(frames, offsets, keep)
    w2 = run[keep].astype(np.int32)
    by_cap = {}
    for cap in CAPS:
        rows, totals = WH.model_records(f2, o2, w2, _T(hvd), cap), WH.model_totals(w2, o2, cap)
        by_cap[cap] = (rows, totals, WH.model_pairs(rows, totals, 50, hvd.vpdq.MATCH_POLICY))
    return f2, o2, w2, dropped, by_cap


@pytest.fixture(scope="module")
def planted(hvd):
    frames, offsets, bases = RH.planted_library()
    RH.assert_far(bases)
    return (frames, offsets) + _model(hvd, frames, offsets)


def test_planted_host_path_under_the_three_caps(gpu, hvd, planted):
    frames, offsets, f2, o2, w2, _, by_cap = planted
    raw_pairs, clean_pairs, _, _ = RH.planted_expectation()
    clean = hvd.without_repeated_frames(RH.blobs(frames, offsets), RH.PLANTED_MAX_DIST)
    assert clean.hashes == RH.blobs(f2, o2) and np.array_equal(np.concatenate(clean.runs), w2)
    cd = (RH.VIDEO_C, RH.VIDEO_D)
    for cap in CAPS:
        rows, totals, pairs = by_cap[cap]
        assert hvd.find_potential_duplicates(clean.hashes, threshold=50, weights=clean.runs, max_weight=cap) == pairs, cap
        recs = hvd.search.match_videos(f2, o2, _T(hvd), weights=clean.runs, max_weight=cap)
        assert WH.rows(recs) == rows, cap
        assert np.array_equal(hvd.search.video_weights(w2, o2, cap), totals), cap
        assert pairs == sorted(raw_pairs if cap == 0 else clean_pairs), cap
        hits = {(a, b): (q, t) for a, b, q, t in rows}[cd]
        assert hits + (int(totals[cd[0]]), int(totals[cd[1]])) == {0: (60, 60, 100, 100), 9: (9, 9, 49, 49), 1: (1, 1, 41, 41)}[cap]
    # uncapped: the totals are the raw lengths; cap 1: the collapsed library's plain search, the existing result
    assert np.array_equal(by_cap[0][1], np.diff(offsets))
    assert by_cap[1][2] == hvd.find_potential_duplicates(clean.hashes, threshold=50)
    assert np.array_equal(hvd.search.match_videos(f2, o2, _T(hvd), weights=clean.runs, max_weight=1),
                          hvd.search.match_videos(f2, o2, _T(hvd)))


def _components(pairs, V):
    """The connected components of two or more nodes, ascending members, sorted by first member."""
    label = list(range(V))
    for _ in range(V):
        for a, b in pairs:
            label[a] = label[b] = min(label[a], label[b])
    groups = {}
    for v in range(V):
        groups.setdefault(label[v], []).append(v)
    return sorted(tuple(m) for m in groups.values() if len(m) > 1)


@pytest.mark.parametrize("cap", CAPS)
def test_groups_of_the_weighted_search_are_the_groups_of_the_models_pairs(gpu, hvd, planted, cap):
    _, _, f2, o2, w2, _, by_cap = planted
    _, totals, pairs = by_cap[cap]
    hashes, weights = RH.blobs(f2, o2), [w2[lo:hi] for lo, hi in zip(o2[:-1], o2[1:])]
    want = _components(pairs, len(o2) - 1)
    assert all(len(m) == 2 for m in want) and len(want) == len(pairs)  # (the planted pairs are disjoint: every group is a pair)
    # default score: the capped weight totals; the larger is kept, ties to the smaller index
    keeper = {m: max(m, key=lambda v: (int(totals[v]), -v)) for m in want}
    groups = hvd.find_duplicate_groups(hashes, threshold=50, weights=weights, max_weight=cap)
    assert [g.members for g in groups] == want and [g.keeper for g in groups] == [keeper[m] for m in want]
    assert all(g.edges == 1 and g.complete for g in groups)
    keepers = hvd.find_keeper_groups(hashes, threshold=50, weights=weights, max_weight=cap)
    assert sorted((g.keeper,) + g.members for g in keepers) == sorted((keeper[m],) + tuple(v for v in m if v != keeper[m]) for m in want)
    if cap == 0:
        assert (RH.VIDEO_C, RH.VIDEO_D) in want and any(totals[a] < totals[b] for a, b in want)  # (a keeper that is not the first)


def test_planted_device_library_under_the_three_caps(gpu, hvd, planted):
    frames, offsets, f2, o2, w2, dropped, by_cap = planted
    source = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        collapsed, got_dropped, d_runs = source.without_repeated_frames(RH.PLANTED_MAX_DIST)
        try:
            collapsed.attach_weights(d_runs)
            assert np.array_equal(got_dropped, dropped) and np.array_equal(collapsed.hashes(), f2)
            for cap in CAPS:
                rows, totals, pairs = by_cap[cap]
                recs = collapsed.match_videos(weighted=True, max_weight=cap)
                assert WH.rows(recs) == rows, cap
                got_totals = collapsed.weight_totals(cap)
                assert got_totals.dtype == np.int64 and np.array_equal(got_totals, totals), cap
                got = hvd.search.similar_video_pairs(recs, got_totals, 50)
                assert [(int(a), int(b)) for a, b in got] == pairs, cap
        finally:
            collapsed.free()
    finally:
        source.free()


def test_planted_frames_through_the_chained_pipeline_weighted(gpu, hvd):
    """The plan as 64 x 64 gray noise images (a held frame is the same image), through hash -> quality filter -> runs ->
    compaction -> weighted search -> totals on one context; the model runs on the product's own hashes of the same frames."""
    plan = RH.planted_plan()
    images = np.random.default_rng(51).integers(0, 256, (RH.planted_scene_count(), 64, 64), dtype=np.uint8)
    flat = np.concatenate([images[video] for video in plan])
    raw_offsets = np.concatenate([[0], np.cumsum([len(video) for video in plan])]).astype(np.int64)
    hashes, quality = hvd.vpdq.hash_frames(flat)
    assert (quality >= hvd.vpdq.QUALITY_TOLERANCE).all()
    _, _, _, want_dropped, by_cap = _model(hvd, hashes, raw_offsets)
    raw_pairs, clean_pairs, _, planted_dropped = RH.planted_expectation()
    assert np.array_equal(want_dropped, planted_dropped)
    d_frames = gpu.DeviceBuffer.from_array(flat)
    try:
        for cap in CAPS:
            rows, _, want_pairs = by_cap[cap]
            pairs, recs, dropped, timings = hvd.pipeline.dedupe_frames_without_repeats_on_device(
                d_frames.ptr, raw_offsets, 64, 64, 1, RH.PLANTED_MAX_DIST, threshold=50, weighted=True, max_weight=cap)
            assert [(int(a), int(b)) for a, b in pairs] == want_pairs == sorted(raw_pairs if cap == 0 else clean_pairs), cap
            assert WH.rows(recs) == rows, cap
            assert dropped.dtype == np.int64 and np.array_equal(dropped, want_dropped)
            assert {"hash_ms", "compact_ms", "runs_ms", "search_ms"} <= set(timings) and "gather_ms" not in timings
        # the plain entry is what it was: the collapsed library's own answer
        pairs, recs, _, _ = hvd.pipeline.dedupe_frames_without_repeats_on_device(d_frames.ptr, raw_offsets, 64, 64, 1,
                                                                                 RH.PLANTED_MAX_DIST, threshold=50)
        assert [(int(a), int(b)) for a, b in pairs] == sorted(clean_pairs) and WH.rows(recs) == by_cap[1][0]
        with pytest.raises(ValueError):
            hvd.pipeline.dedupe_frames_without_repeats_on_device(d_frames.ptr, raw_offsets, 64, 64, 1, RH.PLANTED_MAX_DIST,
                                                                 max_weight=3)  # a cap without weighted=True
    finally:
        d_frames.free()
