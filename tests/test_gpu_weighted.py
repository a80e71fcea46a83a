"""The duration-weighted video search on the GPU, against the numpy model of tests/weighted_helpers.py and against
the plain search: the lossless identity (raw library, plain == max_dist 0 collapse, weights = run), max_weight 1 == the plain
search, random weights at the tolerance edge in the symmetric and the cross form, the regrowth of the pair map, the uint32 edge,
hvd_dev_vpdq_emit_again, k_video_weights at its chunk, ownership and clamp edges, and what a weighted DeviceLibrary carries and
refuses. Every comparison is equality on integers."""
import numpy as np
import pytest

import runs_helpers as RH
import weighted_helpers as WH

pytestmark = pytest.mark.gpu

T = 31  # the frame tolerance of the video search (vpdq.frame_max_dist(search.DISTANCE_TOLERANCE); checked below)
FILL = -7


def _rows(records):
    return WH.rows(records)


def _weighted_library(hvd, gpu, frames, offsets, weights):
    """A DeviceLibrary of a host library with its weights attached (the library owns them)."""
    library = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    library.attach_weights(gpu.DeviceBuffer.from_array(np.ascontiguousarray(weights, np.int32)) if len(weights)
                           else gpu.DeviceBuffer(4))
    return library


def _host_entry(gpu, frames, offsets, weights, max_weight=0, cap=4096):
    """hvd_vpdq_match_videos_weighted itself -> (rows, totals)."""
    import ctypes as C

    off = np.asarray(offsets, np.int64)
    w = np.ascontiguousarray(weights, np.int32)
    out = np.zeros(cap, dtype=[("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4")])
    totals = np.full(off.size - 1, FILL, np.int64)
    cnt = C.c_int64(0)
    gpu.check(gpu.load().hvd_vpdq_match_videos_weighted(frames.ctypes.data, off.ctypes.data, off.size - 1, w.ctypes.data, max_weight,
                                                        T, out.ctypes.data, cap, C.byref(cnt), totals.ctypes.data))
    return _rows(out[:cnt.value]), totals


# ---- 1. the lossless identity ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def held(hvd, gpu):
    assert hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE) == T
    lengths = [130, 0, 200, 64, 7, 1, 90, 45, 150]
    frames, offsets = WH.held_library(lengths, 60, max_hold=[8, 8, 8, 3, 8, 8, 100, 8, 70])
    videos = [frames[lo:hi] for lo, hi in zip(offsets[:-1], offsets[1:])]
    videos.append(np.concatenate([np.repeat(videos[2][:1], 90, axis=0), videos[0][:20]]))  # a hold of 90: past max_run 64
    frames, offsets = RH.library(videos)
    raw =hvd.search.match_videos(frames, offsets, T)
    assert _rows(raw) == WH.model_records(frames, offsets, None, T) and raw.size > 10
    return frames, offsets, raw


@pytest.mark.parametrize("max_run", [0, 1, 2, 64])
def test_lossless_collapse_with_run_weights_gives_the_raw_records(gpu, hvd, held, max_run):
    frames, offsets, raw = held
    lengths = np.diff(offsets)
    clean = hvd.without_repeated_frames(RH.blobs(frames, offsets), 0, max_run)
    f2, o2, w2 = WH.collapse(frames, offsets, max_run)
    assert clean.hashes == RH.blobs(f2, o2) and np.array_equal(np.concatenate(clean.runs), w2)
    assert (len(f2) < len(frames)) == (max_run != 1) and (w2.max() > 64) == (max_run == 0)
    # host route
    got = hvd.search.match_videos(f2, o2, T, weights=clean.runs)
    assert got.dtype == raw.dtype and np.array_equal(got, raw)
    assert np.array_equal(hvd.search.video_weights(w2, o2), lengths)
    rows, totals = _host_entry(gpu, f2, o2, w2)
    assert rows == _rows(raw) and np.array_equal(totals, lengths)
    if max_run != 1:
        assert not np.array_equal(hvd.search.match_videos(f2, o2, T), raw)  # (the plain search of the collapse is another answer)
    # device route: collapse, attach the runs, search
    source = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        collapsed, dropped, d_runs = source.without_repeated_frames(0, max_run)
        try:
            collapsed.attach_weights(d_runs)
            assert np.array_equal(collapsed.match_videos(T, weighted=True), raw)
            assert np.array_equal(collapsed.weight_totals(), lengths) and np.array_equal(dropped, lengths - np.diff(o2))
        finally:
            collapsed.free()
    finally:
        source.free()


# ---- 2. max_weight = 1 -------------------------------------------------------------------------------------------------------

def test_max_weight_1_is_the_plain_search_of_the_same_library(gpu, hvd, held):
    frames, offsets, _ = held
    f2, o2, w2 = WH.collapse(frames, offsets)
    plain = hvd.search.match_videos(f2, o2, T)
    assert np.array_equal(hvd.search.match_videos(f2, o2, T, weights=w2, max_weight=1), plain)
    library = _weighted_library(hvd, gpu, f2, o2, w2)
    try:
        assert np.array_equal(library.match_videos(T, weighted=True, max_weight=1), plain)
        assert np.array_equal(library.match_videos(T), plain)  # attached weights do not touch the plain search
        assert np.array_equal(library.weight_totals(1), np.diff(o2))
    finally:
        library.free()


# ---- 3. against the model: random weights, the tolerance edge, both forms --------------------------------------------------------

CAPS = (0, 1, 3, 1000)


@pytest.mark.parametrize("V", [1, 2, 5, 9])
def test_symmetric_form_against_the_model(gpu, hvd, V):
    frames, offsets, weights = WH.edge_library(V, 70 + V)
    if V > 1:
        at, beyond = WH.edge_distances(frames, offsets, T)
        assert at > 0 and beyond > 0
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    try:
        for cap in CAPS:
            want = WH.model_records(frames, offsets, weights, T, cap)
            assert _rows(hvd.search.match_videos(frames, offsets, T, weights=weights, max_weight=cap)) == want, cap
            assert _rows(library.match_videos(T, weighted=True, max_weight=cap)) == want, cap
            assert np.array_equal(library.weight_totals(cap), WH.model_totals(weights, offsets, cap)), cap
        assert (len(want) > 0) == (V > 1)
    finally:
        library.free()


def _device_cross(gpu, hvd, lq, lt, excl, max_weight):
    """hvd_dev_vpdq_match_videos_cross_weighted of two weighted libraries -> rows sorted by (a, b)."""
    lib = gpu.load()
    d_out, d_cnt = gpu.DeviceBuffer(16 * 4096), gpu.DeviceBuffer(8)
    try:
        gpu.check(lib.hvd_dev_vpdq_match_videos_cross_weighted(
            lq.image().ptr, lq.n_frames, lq.d_video.ptr, lq.d_video.ptr if excl else None, lq.d_weights.ptr,
            lt.image().ptr, lt.n_frames, lt.d_video.ptr, lt.d_video.ptr if excl else None, lt.d_weights.ptr,
            max_weight, T, d_out.ptr, 4096, d_cnt.ptr))
        cnt = int(d_cnt.to_array(np.uint64, 1)[0])
        return sorted(_rows(d_out.to_array(hvd.search.VMATCH_DTYPE, cnt)))
    finally:
        d_out.free()
        d_cnt.free()


@pytest.mark.parametrize("with_ids", [False, True], ids=["all", "ids"])
@pytest.mark.parametrize("V", [1, 2, 5, 9])
def test_cross_form_against_the_model(gpu, hvd, V, with_ids):
    """Different weights on the two sides (1..1000 against 2001..3000 by the offset below): a swapped side shows in every record."""
    fq, oq, wq = WH.edge_library(V, 80 + V, bases_seed=79)
    ft, ot, wt = WH.edge_library(V + 1, 90 + V, bases_seed=79)
    wt = wt + 2000
    ids_q, ids_t = (np.arange(V, dtype=np.int32), np.arange(V + 1, dtype=np.int32)) if with_ids else (None, None)
    lq, lt = _weighted_library(hvd, gpu, fq, oq, wq), _weighted_library(hvd, gpu, ft, ot, wt)
    try:
        for cap in CAPS:
            want = WH.model_records_cross(fq, oq, wq, ft, ot, wt, T, cap, ids_q, ids_t)
            got = hvd.search.match_videos_cross(fq, oq, ft, ot, ids_q, ids_t, T, weights_q=wq, weights_t=wt, max_weight=cap)
            assert _rows(got) == want, cap
            # (on the device the frame -> video maps are the exclusion maps: equal video indices are not compared)
            assert _device_cross(gpu, hvd, lq, lt, with_ids, cap) == want, cap
        assert len(want) > 0
        if not with_ids:  # q_hits is a sum of query weights (each <= 1000 per frame), t_hits of target weights (each > 2000)
            uncapped = WH.model_records_cross(fq, oq, wq, ft, ot, wt, T)
            assert all(t > 2000 for _, _, _, t in uncapped) and uncapped != [(a, b, t, q) for a, b, q, t in uncapped]
    finally:
        lq.free()
        lt.free()


# ---- 4. regrowth of the pair map ---------------------------------------------------------------------------------------------

def test_a_regrown_pair_map_does_not_count_twice(gpu, hvd):
    """Tables that start at 16 slots: more than 16 video pairs cannot fit, the fold fails, both tables are cleared and the pass
    runs again at four times the size -- with sums of weights where a second pass on uncleared counters would show."""
    frames, offsets, weights = WH.edge_library(9, 79)
    want = WH.model_records(frames, offsets, weights, T)
    assert len(want) > 16
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    lib = gpu.load()
    try:
        gpu.check(lib.hvd_debug_set(b"vmatch_slots_log2", 4))
        assert _rows(library.match_videos(T, weighted=True)) == want
        assert _rows(hvd.search.match_videos(frames, offsets, T, weights=weights)) == want
        assert _rows(library.match_videos(T, weighted=True, max_weight=3)) == WH.model_records(frames, offsets, weights, T, 3)
    finally:
        gpu.check(lib.hvd_debug_set(b"vmatch_slots_log2", 0))
        library.free()


# ---- 5. the uint32 edge ------------------------------------------------------------------------------------------------------

def test_counters_reach_2_32_minus_1(gpu, hvd):
    big = (1 << 31) - 1
    video = RH.random_hashes(3, 81)
    RH.assert_far(video)
    frames, offsets = RH.library([video, video])
    weights = np.array([big, big, 1] * 2, dtype=np.int32)
    want = [(0, 1, (1 << 32) - 1, (1 << 32) - 1)]
    assert _rows(hvd.search.match_videos(frames, offsets, T, weights=weights)) == want
    rows, totals = _host_entry(gpu, frames, offsets, weights)
    assert rows == want and totals.tolist() == [(1 << 32) - 1] * 2
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    try:
        assert _rows(library.match_videos(T, weighted=True)) == want
        assert library.weight_totals().tolist() == [(1 << 32) - 1] * 2
    finally:
        library.free()
    # one more and the host entry refuses; the device library's totals do
    weights[2] = 2
    with pytest.raises(ValueError, match="video 0"):
        hvd.search.match_videos(frames, offsets, T, weights=weights)
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    try:
        with pytest.raises(ValueError, match="video 0"):
            library.weight_totals()
        assert library.weight_totals(5).tolist() == [12, 11]  # (5 + 5 + 2, 5 + 5 + 1)
    finally:
        library.free()


# ---- 6. hvd_dev_vpdq_emit_again ----------------------------------------------------------------------------------------------

def test_emit_again_returns_the_weighted_records(gpu, hvd):
    frames, offsets, weights = WH.edge_library(9, 82)
    want = WH.model_records(frames, offsets, weights, T, 7)
    assert len(want) > 4
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    lib = gpu.load()
    d_small, d_large, d_cnt = gpu.DeviceBuffer(16 * 2), gpu.DeviceBuffer(16 * 4096), gpu.DeviceBuffer(8)
    try:
        gpu.check(lib.hvd_dev_vpdq_match_videos_weighted(library.image().ptr, library.n_frames, library.d_video.ptr,
                                                         library.d_weights.ptr, 7, T, d_small.ptr, 2, d_cnt.ptr))
        assert int(d_cnt.to_array(np.uint64, 1)[0]) == len(want)  # the true count, two records written
        gpu.check(lib.hvd_dev_vpdq_emit_again(d_large.ptr, 4096, d_cnt.ptr))
        cnt = int(d_cnt.to_array(np.uint64, 1)[0])
        assert sorted(_rows(d_large.to_array(hvd.search.VMATCH_DTYPE, cnt))) == want
        # the Python route takes the same path when its buffer is too small
        assert _rows(library.match_videos(T, cap=2, weighted=True, max_weight=7)) == want
    finally:
        for b in (d_small, d_large, d_cnt):
            b.free()
        library.free()


# ---- 7. k_video_weights ------------------------------------------------------------------------------------------------------

def _device_totals(gpu, weights, offsets, max_weight=0, n=None):
    """hvd_dev_video_weights over a buffer that holds every weight (n: the frame count passed, default all), the output filled
    with FILL beforehand."""
    total, V = len(weights), len(offsets) - 1
    n = total if n is None else n
    d_w = gpu.DeviceBuffer.from_array(np.ascontiguousarray(weights, np.int32)) if total else gpu.DeviceBuffer(4)
    d_o = gpu.DeviceBuffer.from_array(np.asarray(offsets, np.int64))
    d_t = gpu.DeviceBuffer.from_array(np.full(max(V, 1), FILL, np.int64))
    try:
        gpu.check(gpu.load().hvd_dev_video_weights(d_w.ptr, d_o.ptr, V, n, max_weight, d_t.ptr))
        return d_t.to_array(np.int64, V)
    finally:
        gpu.check(gpu.load().hvd_dev_sync())
        for b in (d_w, d_o, d_t):
            b.free()


def _clamped_totals(weights, offsets, max_weight, n):
    w = WH.capped(weights, max_weight)
    return np.array([w[min(lo, min(hi, n)):min(hi, n)].sum() for lo, hi in zip(offsets[:-1], offsets[1:])], dtype=np.int64)


WEIGHT_SHAPES = {
    "chunks": [0, 0, 1, 63, 64, 0, 65, 129, 200, 0],  # every chunk edge; empty videos at both ends and in the middle
    "V1": [129], "V3": [64, 0, 1], "V4": [1, 200, 0, 63], "V5": [0, 65, 2, 64, 0],
}


@pytest.mark.parametrize("shape", list(WEIGHT_SHAPES))
def test_video_weights_at_chunk_and_ownership_edges(gpu, shape):
    lengths = WEIGHT_SHAPES[shape]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rng = np.random.default_rng(83)
    small = rng.integers(1, 6, int(offsets[-1])).astype(np.int32)
    large = np.full(int(offsets[-1]), (1 << 31) - 1, np.int32)  # 64-bit sums: 200 of these are past 2^38
    for cap in (0, 1, 2):
        assert np.array_equal(_device_totals(gpu, small, offsets, cap), WH.model_totals(small, offsets, cap)), cap
        assert np.array_equal(_device_totals(gpu, large, offsets, cap), WH.model_totals(large, offsets, cap)), cap
    assert np.array_equal(_device_totals(gpu, small, offsets, 1), np.asarray(lengths))


def test_video_weights_past_one_grid(gpu):
    V = 4 * 1024 + 7
    rng = np.random.default_rng(84)
    lengths = rng.integers(1, 4, V)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    weights = rng.integers(1, 1001, int(offsets[-1])).astype(np.int32)
    for cap in (0, 2):
        assert np.array_equal(_device_totals(gpu, weights, offsets, cap), WH.model_totals(weights, offsets, cap)), cap


def test_video_weights_clamps_offsets_past_n(gpu):
    lengths = [5, 70, 0, 130, 64, 3]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    weights = np.random.default_rng(85).integers(1, 1001, int(offsets[-1])).astype(np.int32)
    for n in (int(offsets[-1]) - 1, 205, 140, 75, 5, 0):  # inside the last video, ..., at a boundary, nothing at all
        for cap in (0, 1, 2):
            want = _clamped_totals(weights, offsets, cap, n)
            assert np.array_equal(_device_totals(gpu, weights, offsets, cap, n=n), want), (n, cap)
    assert _device_totals(gpu, np.zeros(0, np.int32), [0, 0, 0], 0).tolist() == [0, 0]
    assert _device_totals(gpu, np.zeros(0, np.int32), [0], 0).size == 0


# ---- 8. what a weighted library carries and refuses ---------------------------------------------------------------------------

def test_without_common_frames_carries_the_weights(gpu, hvd):
    rng = np.random.default_rng(86)
    logo = RH.random_hashes(1, 87)
    videos = [np.concatenate([logo, RH.random_hashes(int(k), 88 + i)]) for i, k in enumerate((6, 4, 9, 5, 7))]
    frames, offsets = RH.library(videos)
    weights = rng.integers(1, 1001, len(frames)).astype(np.int32)
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    try:
        filtered, dropped = library.without_common_frames(2, 50, T)
        try:
            assert dropped.tolist() == [1] * 5 and filtered.d_weights is not None and filtered.d_weights is not library.d_weights
            kept = np.ones(len(frames), bool)
            kept[offsets[:-1]] = False
            assert np.array_equal(filtered.hashes(), frames[kept])
            assert np.array_equal(filtered.d_weights.to_array(np.int32, filtered.n_frames), weights[kept])
            assert np.array_equal(filtered.weight_totals(), WH.model_totals(weights[kept], filtered.offsets()))
            assert _rows(filtered.match_videos(T, weighted=True)) == WH.model_records(frames[kept], filtered.offsets(), weights[kept], T)
        finally:
            filtered.free()
        plain = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
        try:
            unweighted, _ = plain.without_common_frames(2, 50, T)
            assert unweighted.d_weights is None
            unweighted.free()
        finally:
            plain.free()
    finally:
        library.free()


def test_a_weighted_library_refuses_what_would_drop_its_weights(gpu, hvd):
    frames, offsets, weights = WH.edge_library(3, 89)
    library = _weighted_library(hvd, gpu, frames, offsets, weights)
    other = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        with pytest.raises(ValueError, match="weights"):
            library.without_repeated_frames(0)
        with pytest.raises(ValueError, match="weights"):
            library.extended(other)
        with pytest.raises(ValueError, match="weights"):
            other.extended(library)
        with pytest.raises(ValueError, match="weights"):
            library.ingest(other)
        with pytest.raises(ValueError, match="weights"):
            other.ingest(library)
        # the weighted search needs weights and one context
        with pytest.raises(ValueError):
            other.match_videos(T, weighted=True)
        with pytest.raises(ValueError):
            other.weight_totals()
        with pytest.raises(ValueError):
            library.match_videos(T, world=2, weighted=True)
        with pytest.raises(ValueError):
            library.match_videos(T, weighted=True, max_weight=-1)
        d_small = gpu.DeviceBuffer(4)
        with pytest.raises(ValueError):
            library.attach_weights(d_small)  # too small: not taken over
        d_small.free()
        # both still work
        assert _rows(library.match_videos(T, weighted=True)) == WH.model_records(frames, offsets, weights, T)
        assert _rows(other.match_videos(T)) == WH.model_records(frames, offsets, None, T)
    finally:
        library.free()
        other.free()
