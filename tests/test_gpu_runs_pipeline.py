"""The static-scene filter end to end on the GPU, on the planted library of tests/runs_helpers.py: six sources of
20 scenes, each as a video A that holds every scene 1..9 frames and as a video B with other hold lengths; two otherwise
unrelated videos C and D of 100 frames that share one scene held for 60; three unrelated videos. The raw search reports the six
copies and (C, D); after the collapse at max_dist 8 every A and B has 20 frames, C and D have 41, and the search reports the six
copies alone. tests/test_runs_cpu.py checks the same expectations by the model and the oracle."""
import numpy as np
import pytest

import runs_helpers as RH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planted(hvd, oracle):
    frames, offsets, bases = RH.planted_library()
    RH.assert_far(bases)
    keep, run = RH.model_runs(frames, offsets, RH.PLANTED_MAX_DIST)
    return frames, offsets, keep, run, RH.model_collapsed(frames, offsets, keep)


def _T(hvd):
    return hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)


def test_planted_host_path(gpu, hvd, oracle, planted):
    frames, offsets, keep, run, (f2, o2, pos2, _) = planted
    raw_pairs, clean_pairs, want_kept, want_dropped = RH.planted_expectation()
    hashes = RH.blobs(frames, offsets)
    assert hvd.find_potential_duplicates(hashes, threshold=50) == sorted(raw_pairs)  # the problem: (C, D) is reported
    clean = hvd.without_repeated_frames(hashes, RH.PLANTED_MAX_DIST)
    assert clean.hashes == RH.blobs(f2, o2)
    assert [len(b) // 32 for b in clean.hashes] == want_kept.tolist() and want_kept[:12].tolist() == [20] * 12
    assert want_kept[RH.VIDEO_C] == want_kept[RH.VIDEO_D] == 41
    assert np.array_equal(clean.dropped, want_dropped)
    assert np.array_equal(np.concatenate(clean.positions), pos2) and np.array_equal(np.concatenate(clean.runs), run[keep])
    got = hvd.find_potential_duplicates(clean.hashes, threshold=50)
    assert got == RH.model_pairs(oracle, f2, o2, _T(hvd), 50, hvd) == sorted(clean_pairs)
    assert (RH.VIDEO_C, RH.VIDEO_D) not in got


def test_excerpts_of_the_collapsed_library_are_on_the_raw_timeline(gpu, hvd, planted):
    """An excerpt cut from A_0 at scene boundaries (scenes 5..14, the holds as they are) next to the planted library: after the
    collapse its ten frames align with A_0's at the RAW index at which scene 5 starts there, not at 5."""
    frames, offsets, _, _, _ = planted
    plan = RH.planted_plan()
    a0 = plan[0]
    cut_lo, cut_hi = a0.index(5), a0.index(15)
    hashes = RH.blobs(frames, offsets) + [frames[cut_lo:cut_hi].tobytes()]
    E = len(hashes) - 1
    clean = hvd.without_repeated_frames(hashes, RH.PLANTED_MAX_DIST)
    assert len(clean.hashes[E]) // 32 == 10 and len(clean.hashes[0]) // 32 == 20
    excerpts = hvd.find_excerpts(clean.hashes, positions=clean.positions)
    by_pair = {(e.short, e.long): e for e in excerpts}
    e = by_pair[(E, 0)]
    assert cut_lo > 5 and e.offset == cut_lo and e.first == cut_lo and e.last == a0.index(14) and int(e.coverage) == 100
    for e in excerpts:  # every reported place is the raw position of a kept frame of the long video
        assert e.first in clean.positions[e.long] and e.last in clean.positions[e.long]
    # without the positions the same excerpt sits at the collapsed index
    assert {(x.short, x.long): x for x in hvd.find_excerpts(clean.hashes)}[(E, 0)].offset == 5


def test_planted_device_library(gpu, hvd, oracle, planted):
    frames, offsets, keep, run, (f2, o2, pos2, _) = planted
    _, clean_pairs, want_kept, want_dropped = RH.planted_expectation()
    source = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        collapsed, dropped, d_runs = source.without_repeated_frames(RH.PLANTED_MAX_DIST)
        try:
            assert np.array_equal(dropped, want_dropped) and np.array_equal(collapsed.lengths(), want_kept)
            assert np.array_equal(collapsed.hashes(), f2) and np.array_equal(collapsed.positions(), pos2)
            assert np.array_equal(d_runs.to_array(np.int32, collapsed.n_frames), run[keep])
            recs = collapsed.match_videos()
            assert np.array_equal(recs, oracle.match_videos(f2, o2, _T(hvd)))
            pairs = hvd.search.similar_video_pairs(recs, collapsed.lengths(), 50)
            assert [(int(a), int(b)) for a, b in pairs] == sorted(clean_pairs)
        finally:
            d_runs.free()
            collapsed.free()
    finally:
        source.free()


def test_planted_frames_through_the_chained_pipeline(gpu, hvd):
    """The same plan as 64 x 64 gray images (random noise: high PDQ quality, unrelated hashes; a held frame is the same image),
    through hash -> quality filter -> runs -> compaction -> search on one context, against the host route on the product's
    own hashes of the same frames."""
    plan = RH.planted_plan()
    images = np.random.default_rng(51).integers(0, 256, (RH.planted_scene_count(), 64, 64), dtype=np.uint8)
    flat = np.concatenate([images[video] for video in plan])
    raw_offsets = np.concatenate([[0], np.cumsum([len(video) for video in plan])]).astype(np.int64)
    hashes, quality = hvd.vpdq.hash_frames(flat)
    assert (quality >= hvd.vpdq.QUALITY_TOLERANCE).all()  # (noise has quality 100: the scenario is the planted one)
    raw_pairs, clean_pairs, want_kept, want_dropped = RH.planted_expectation()
    host = hvd.without_repeated_frames(RH.blobs(hashes, raw_offsets), RH.PLANTED_MAX_DIST)
    host_pairs = hvd.find_potential_duplicates(host.hashes, threshold=50)
    assert np.array_equal(host.dropped, want_dropped) and host_pairs == sorted(clean_pairs)
    d_frames = gpu.DeviceBuffer.from_array(flat)
    try:
        pairs, recs, dropped, timings = hvd.pipeline.dedupe_frames_without_repeats_on_device(
            d_frames.ptr, raw_offsets, 64, 64, 1, RH.PLANTED_MAX_DIST, threshold=50)
        assert [(int(a), int(b)) for a, b in pairs] == host_pairs
        assert dropped.dtype == np.int64 and np.array_equal(dropped, host.dropped)
        assert {"hash_ms", "compact_ms", "runs_ms", "search_ms"} <= set(timings) and "gather_ms" not in timings
        unfiltered, _, _ = hvd.pipeline.dedupe_frames_on_device(d_frames.ptr, raw_offsets, 64, 64, 1, threshold=50)
        assert [(int(a), int(b)) for a, b in unfiltered] == sorted(raw_pairs)
    finally:
        d_frames.free()
