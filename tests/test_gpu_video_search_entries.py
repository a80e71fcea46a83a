"""The twelve video-search entries of the C-ABI on one library: the eight searches must give the records of
tests/weighted_helpers.py's model, the four spreads the counts of tests/spread_helpers.py's -- whichever entry, host or device,
plain or weighted at unit weights, one side or two. And the popcount route of hvd_vpdq_match_videos (max_dist 128..256), which
no other test drives."""
import numpy as np
import pytest

import ingest_helpers as IH
import spread_helpers as SH
import weighted_helpers as WH

T = 31  # the frame tolerance of the video search: edge_library puts frame pairs at T and at T + 1
POPCOUNT_LENGTHS = (0, 7, 1, 12, 20)
POPCOUNT_TOLERANCES = (128, 200, 256)


def popcount_library():
    """Five videos, two of them with nothing or one frame, 40 random frames: pairs lie around 128 bits apart (sd 8)."""
    offsets = np.concatenate([[0], np.cumsum(POPCOUNT_LENGTHS)]).astype(np.int64)
    return SH.random_hashes(int(offsets[-1]), 4022), offsets


def test_model_and_oracle_agree_on_the_popcount_tolerances(oracle):
    """(no GPU: the two references of the test below, held against each other before either is relied on)"""
    frames, offsets = popcount_library()
    for tol in POPCOUNT_TOLERANCES:
        assert WH.rows(oracle.match_videos(frames, offsets, tol)) == WH.model_records(frames, offsets, None, tol), tol
    # 128 is neither a tolerance at which nothing matches nor one at which every frame does: the counters are worth comparing
    at_128 = WH.model_records(frames, offsets, None, 128)
    assert at_128 and any(q < POPCOUNT_LENGTHS[a] or t < POPCOUNT_LENGTHS[b] for a, b, q, t in at_128)


@pytest.mark.gpu
@pytest.mark.parametrize("tol", POPCOUNT_TOLERANCES)
def test_popcount_route_against_the_model(gpu, hvd, tol):
    frames, offsets = popcount_library()
    got = WH.rows(hvd.search.match_videos(frames, offsets, tol))
    assert got == WH.model_records(frames, offsets, None, tol)
    if tol == 256:  # every frame matches every frame: each pair of videos that have frames, with their lengths
        n = POPCOUNT_LENGTHS
        assert got == [(a, b, n[a], n[b]) for a in range(5) for b in range(a + 1, 5) if n[a] and n[b]]


def _device_records(gpu, hvd, launch, cap=4096):
    return WH.rows(hvd.pipeline._search_records(launch, cap))


@pytest.mark.gpu
@pytest.mark.parametrize("V", [9, 1, 2])
def test_every_search_entry_gives_the_model_records(gpu, hvd, V):
    frames, offsets, _ = WH.edge_library(V, 300 + V)
    want = WH.model_records(frames, offsets, None, T)
    assert V < 9 or (min(WH.edge_distances(frames, offsets, T)) > 0 and len(want) > 5)
    ones, ids = np.ones(len(frames), np.int32), np.arange(V, dtype=np.int32)
    S = hvd.search

    def upper(rows):  # a library against itself without equal ids: both (a, b) and (b, a); a < b is the symmetric record set
        assert sorted((b, a, t, q) for a, b, q, t in rows if a > b) == [r for r in rows if r[0] < r[1]]
        return [r for r in rows if r[0] < r[1]]

    assert WH.rows(S.match_videos(frames, offsets, T)) == want
    assert WH.rows(S.match_videos(frames, offsets, T, weights=ones)) == want
    assert upper(WH.rows(S.match_videos_cross(frames, offsets, frames, offsets, ids, ids, T))) == want
    assert upper(WH.rows(S.match_videos_cross(frames, offsets, frames, offsets, ids, ids, T, weights_q=ones, weights_t=ones))) == want
    library = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    queries = hvd.pipeline.DeviceQueries(gpu.DeviceBuffer.from_array(frames), gpu.DeviceBuffer.from_array(SH.video_of(offsets)),
                                         gpu.DeviceBuffer.from_array(SH.video_of(offsets)), len(frames), V, ("same",))
    try:
        library.attach_weights(gpu.DeviceBuffer.from_array(ones))
        assert WH.rows(library.match_videos(T)) == want
        assert WH.rows(library.match_videos(T, weighted=True)) == want
        assert upper(WH.rows(library.match_queries(queries, T))) == want
        lib, img, vid, w, n = gpu.load(), library.image().ptr, library.d_video.ptr, library.d_weights.ptr, library.n_frames
        assert upper(_device_records(gpu, hvd, lambda d_out, cap, d_cnt: lib.hvd_dev_vpdq_match_videos_cross_weighted(
            img, n, vid, vid, w, img, n, vid, vid, w, 0, T, d_out, cap, d_cnt))) == want
    finally:
        library.free()
        queries.free()


@pytest.mark.gpu
@pytest.mark.parametrize("V", [9, 1, 2])
def test_every_spread_entry_gives_the_model_counts(gpu, hvd, oracle, V):
    """The rectangle by the model's additivity: the library cut in two, T = the first videos and Q = the rest; the spread of
    the whole is each side's own plus what the other side adds."""
    frames, offsets, _ = WH.edge_library(V, 300 + V)
    whole = SH.model_spread(oracle, frames, offsets, T)
    assert V < 9 or whole.max() >= 2
    (ft, ot), (fq, oq) = IH.cut(frames, offsets, 0, V // 2), IH.cut(frames, offsets, V // 2, V)
    want_t = whole[:len(ft)] - SH.model_spread(oracle, ft, ot, T)
    want_q = whole[len(ft):] - SH.model_spread(oracle, fq, oq, T)
    assert V < 9 or (want_t.any() and want_q.any())
    assert np.array_equal(hvd.search.frame_spread(frames, offsets, T), whole)
    sq, st = hvd.search.frame_spread_cross(fq, oq, ft, ot, T)
    assert np.array_equal(sq, want_q) and np.array_equal(st, want_t)
    P = hvd.pipeline.DeviceLibrary
    library, lt, lq = P.from_host(frames, offsets), P.from_host(ft, ot), P.from_host(fq, oq)
    buffers = []
    try:
        buffers.append(library.spread(T))
        assert np.array_equal(buffers[0].to_array(np.int32, len(frames)), whole)
        buffers += lt.spread_cross(lq, T)
        assert np.array_equal(buffers[1].to_array(np.int32, len(fq)), want_q)
        assert np.array_equal(buffers[2].to_array(np.int32, len(ft)), want_t)
    finally:
        for x in [library, lt, lq] + buffers:
            x.free()
