"""The static-scene filter on the GPU: k_frame_runs through hvd_dev_frame_runs on device buffers and through the
host entry hvd_vpdq_frame_runs, against the plain loop of tests/runs_helpers.py -- `keep` and `run` word for word -- at the
chunk edges, the tolerance edge, every max_run path, every ownership shape, with a null run pointer and with offsets past n;
then DeviceLibrary.without_repeated_frames against search.without_repeated_frames. Every comparison is equality on integers."""
import os
import re

import numpy as np
import pytest

import runs_helpers as RH
from conftest import ROOT

pytestmark = pytest.mark.gpu

FILL = -7


def _device_runs(gpu, frames, offsets, max_dist, max_run=0, with_run=True, n=None):
    """hvd_dev_frame_runs over buffers that hold every frame of `frames` (n: the frame count passed, default all of them),
    the outputs filled with FILL beforehand -> (keep int32, run int32), as long as `frames`; with_run=False passes no run
    buffer and returns the untouched one."""
    total, V = len(frames), len(offsets) - 1
    n = total if n is None else n
    d_h = gpu.DeviceBuffer.from_array(np.ascontiguousarray(frames, np.uint8)) if total else gpu.DeviceBuffer(32)
    d_o = gpu.DeviceBuffer.from_array(np.asarray(offsets, np.int64))
    d_k = gpu.DeviceBuffer.from_array(np.full(max(total, 1), FILL, np.int32))
    d_r = gpu.DeviceBuffer.from_array(np.full(max(total, 1), FILL, np.int32))
    try:
        gpu.check(gpu.load().hvd_dev_frame_runs(d_h.ptr, d_o.ptr, V, n, max_dist, max_run, d_k.ptr, d_r.ptr if with_run else None))
        return d_k.to_array(np.int32, total), d_r.to_array(np.int32, total)
    finally:
        gpu.check(gpu.load().hvd_dev_sync())
        for b in (d_h, d_o, d_k, d_r):
            b.free()


def _assert_equals_model(gpu, hvd, frames, offsets, max_dist, max_run=0, what=""):
    want_keep, want_run = RH.model_runs(frames, offsets, max_dist, max_run)
    keep, run = _device_runs(gpu, frames, offsets, max_dist, max_run)
    assert np.array_equal(keep, want_keep.astype(np.int32)), (what, "keep, device entry")
    assert np.array_equal(run, want_run), (what, "run, device entry")
    host_keep, host_run = hvd.search.frame_runs(frames, offsets, max_dist, max_run)
    assert host_keep.dtype == bool and host_run.dtype == np.int32
    assert np.array_equal(host_keep, want_keep) and np.array_equal(host_run, want_run), (what, "host entry")
    return want_keep, want_run


CHUNK_LENGTHS = (0, 1, 2, 63, 64, 65, 66, 128, 129, 130, 193)


# ---- 1. chunk edges ----------------------------------------------------------------------------------------------------------

def test_one_run_over_every_chunk(gpu, hvd):
    x = RH.random_hashes(1, 31)
    for length in CHUNK_LENGTHS:
        keep, run = _assert_equals_model(gpu, hvd, np.repeat(x, length, axis=0), [0, length], 8, what=length)
        assert keep.tolist() == [True] + [False] * (length - 1) if length else keep.size == 0
        assert run[:1].tolist() == [length][:length]


def test_sixty_four_new_anchors_per_chunk(gpu, hvd):
    frames = RH.random_hashes(193, 32)
    RH.assert_far(frames)
    for length in CHUNK_LENGTHS:
        keep, run = _assert_equals_model(gpu, hvd, frames[:length], [0, length], 31, what=length)
        assert keep.all() and (run == 1).all()


@pytest.mark.parametrize("prefix", [0, 63], ids=["lane0", "lane63"])
@pytest.mark.parametrize("order", ["up", "down", "mixed"])
def test_planted_runs_start_at_either_end_of_a_chunk_and_cross_chunk_ends(gpu, hvd, prefix, order):
    """Runs of 1, 2, 63, 64, 65, 127 and 128 frames behind `prefix` single frames: the first run starts at lane 0 or at lane 63
    of a chunk; the others start wherever the lengths before them put them, and the long ones span two and three chunks."""
    lengths = {"up": RH.PLANTED_RUNS, "down": RH.PLANTED_RUNS[::-1], "mixed": (64, 1, 128, 63, 2, 127, 65)}[order]
    video = RH.run_video(lengths, 8, np.random.default_rng(33 + prefix), prefix=prefix)
    RH.assert_far(video[np.concatenate([np.arange(prefix), prefix + np.cumsum((0,) + lengths[:-1])]).astype(int)])
    keep, run = _assert_equals_model(gpu, hvd, video, [0, len(video)], 8, what=(prefix, order))
    assert run[keep].tolist() == [1] * prefix + list(lengths)
    ends = prefix + np.cumsum(lengths)
    assert ((ends - 1) // 64 > (ends - np.asarray(lengths)) // 64).sum() >= 3  # (runs that reach into a later chunk)


# ---- 2. tolerance edge ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_dist", [0, 1, 30, 31, 32, 127])
def test_frames_at_and_just_beyond_the_tolerance(gpu, hvd, max_dist):
    x = RH.random_hashes(1, 34)[0]
    at = RH.flipped(x, range(max_dist))                       # exactly max_dist from x: dropped
    beyond = RH.flipped(x, range(100, 100 + max_dist + 1))    # max_dist + 1 from x: kept, the new anchor
    video = np.stack([x, at, beyond, RH.flipped(beyond, range(max_dist)), RH.flipped(beyond, range(max_dist + 1)), x])
    assert RH.hamming(x, at) == max_dist and RH.hamming(x, beyond) == max_dist + 1
    keep, run = _assert_equals_model(gpu, hvd, video, [0, 6], max_dist, what=max_dist)
    # (the last frame is x again: max_dist + 1 + max_dist + 1 bits from its anchor, the fifth frame)
    assert keep.tolist() == [True, False, True, False, True, True] and run.tolist() == [2, 0, 2, 0, 1, 1]


def test_drift_cannot_chain_a_video_into_one_run(gpu, hvd):
    x = RH.random_hashes(1, 35)[0]
    drift = [x]
    for i in range(1, 80):
        drift.append(RH.flipped(drift[-1], range(3 * i, 3 * i + 3)))  # 3 fresh bits per frame: 9 > 8 at every third
    keep, run = _assert_equals_model(gpu, hvd, np.stack(drift), [0, 80], 8)
    assert keep.tolist() == [i % 3 == 0 for i in range(80)]


def test_a_frame_is_judged_against_its_anchor_not_its_predecessor(gpu, hvd):
    x = RH.random_hashes(1, 36)[0]
    video = np.stack([x, RH.flipped(x, range(0, 8)), RH.flipped(x, range(100, 108)), RH.flipped(x, range(0, 9))])
    assert RH.hamming(video[1], video[2]) == 16 and RH.hamming(video[2], video[3]) == 17
    keep, run = _assert_equals_model(gpu, hvd, video, [0, 4], 8)
    assert keep.tolist() == [True, False, False, True] and run.tolist() == [3, 0, 0, 1]


# ---- 3. max_run ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_run", [0, 1, 2, 63, 64, 65, 200])
def test_max_run_on_an_all_equal_video_and_on_the_planted_runs(gpu, hvd, max_run):
    x = RH.random_hashes(1, 37)
    keep, run = _assert_equals_model(gpu, hvd, np.repeat(x, 300, axis=0), [0, 300], 8, max_run, what="equal")
    full = max_run if max_run else 300
    assert run[keep].tolist() == [full] * (300 // full) + [300 % full] * (300 % full > 0)
    for prefix in (0, 63):
        video = RH.run_video(RH.PLANTED_RUNS, 8, np.random.default_rng(38 + prefix), prefix=prefix)
        keep, run = _assert_equals_model(gpu, hvd, video, [0, len(video)], 8, max_run, what=("planted", prefix))
        assert max_run == 0 or run.max() <= max_run
        assert max_run != 1 or keep.all()


# ---- 4. ownership ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 3, 4, 5, 9])
def test_videos_of_different_lengths_over_the_waves_of_a_workgroup(gpu, hvd, V):
    lengths = np.random.default_rng(40 + V).choice([1, 2, 40, 64, 65, 150, 200], V)
    lengths[0] = 150
    frames, offsets = RH.mixed_library(lengths, 8, 41 + V)
    keep, _ = _assert_equals_model(gpu, hvd, frames, offsets, 8, what=lengths.tolist())
    assert keep[offsets[:-1]].all() and not keep.all()
    _assert_equals_model(gpu, hvd, frames, offsets, 8, 5, what=lengths.tolist())


@pytest.mark.parametrize("lengths", [[0, 0, 70, 3], [5, 0, 0, 0, 0, 130], [64, 1, 0, 0], [0, 9, 0, 0, 0, 0, 0, 0, 66, 0], [0], [0, 0, 0, 0, 0]],
                         ids=lambda x: "-".join(map(str, x)))
def test_empty_videos_at_both_ends_and_in_the_middle(gpu, hvd, lengths):
    frames, offsets = RH.mixed_library(lengths, 8, 42 + len(lengths))
    _assert_equals_model(gpu, hvd, frames, offsets, 8, what=lengths)


def test_more_groups_of_four_than_the_grid_has_workgroups(gpu, hvd):
    """The launch is capped at kFrameRunsMaxBlocks workgroups of four videos: ten groups more, and the first ten workgroups take
    a second trip -- to videos longer than a chunk, so that a trip that never happened cannot go unseen."""
    text = open(os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "hvd_kernels.h")).read()
    cap = int(re.search(r"constexpr unsigned kFrameRunsMaxBlocks = (\d+);", text).group(1))
    rng = np.random.default_rng(43)
    lengths = np.concatenate([rng.integers(0, 3, 4 * cap), rng.integers(60, 71, 38)])  # (the last group holds two videos)
    assert (len(lengths) + 3) // 4 == cap + 10 and lengths.sum() < 8 * cap
    frames, offsets = RH.mixed_library(lengths, 8, 44)
    keep, run = _assert_equals_model(gpu, hvd, frames, offsets, 8)
    assert not keep[offsets[4 * cap]:].all()


# ---- 5. a null run pointer ---------------------------------------------------------------------------------------------------

def test_without_a_run_buffer_the_flags_are_the_same(gpu):
    frames, offsets = RH.mixed_library([70, 0, 131, 5, 64], 8, 45)
    for max_run in (0, 3):
        keep, run = _device_runs(gpu, frames, offsets, 8, max_run, with_run=False)
        assert np.array_equal(keep, RH.model_runs(frames, offsets, 8, max_run)[0].astype(np.int32))
        assert (run == FILL).all()  # (the buffer that was not passed is not written)


# ---- 6. offsets past n are clamped -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("offsets,n", [([0, 50, 200], 120), ([0, 50, 130, 200], 120), ([0, 200], 64), ([0, 10, 200], 10)],
                         ids=["last-cut", "one-beyond", "chunk-end", "at-n"])
def test_ranges_are_clamped_to_the_frame_count(gpu, offsets, n):
    """offsets[V] is larger than n. Hashes and outputs are allocated for the unclamped range, so even a kernel without the clamp
    would stay inside its allocations; the words from n on must be untouched."""
    frames, _ = RH.mixed_library([200], 8, 46)
    keep, run = _device_runs(gpu, frames, offsets, 8, 0, n=n)
    clamped = np.minimum(np.asarray(offsets), n)
    want_keep, want_run = RH.model_runs(frames[:n], clamped, 8, 0)
    assert np.array_equal(keep[:n], want_keep.astype(np.int32)) and np.array_equal(run[:n], want_run)
    assert (keep[n:] == FILL).all() and (run[n:] == FILL).all()


def test_bad_arguments_are_refused_and_nothing_is_launched(gpu, hvd):
    lib = gpu.load()
    frames, offsets = np.repeat(RH.random_hashes(1, 47), 4, axis=0), np.array([0, 4], np.int64)
    d_h, d_o = gpu.DeviceBuffer.from_array(frames), gpu.DeviceBuffer.from_array(offsets)
    d_k = gpu.DeviceBuffer.from_array(np.full(4, FILL, np.int32))
    try:
        for max_dist, max_run, V, n in ((-1, 0, 1, 4), (128, 0, 1, 4), (8, -1, 1, 4), (8, (1 << 20) + 1, 1, 4), (8, 0, -1, 4), (8, 0, 1, -1)):
            assert lib.hvd_dev_frame_runs(d_h.ptr, d_o.ptr, V, n, max_dist, max_run, d_k.ptr, None) == gpu.HVD_ERR_ARG
        gpu.check(lib.hvd_dev_sync())
        assert d_k.to_array(np.int32, 4).tolist() == [FILL] * 4
        gpu.check(lib.hvd_dev_frame_runs(d_h.ptr, d_o.ptr, 1, 4, 127, 1 << 20, d_k.ptr, None))  # (and the good call does write)
        assert d_k.to_array(np.int32, 4).tolist() == [1, 0, 0, 0]
    finally:
        for b in (d_h, d_o, d_k):
            b.free()
    library = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        for max_dist, max_run in ((128, 0), (8, -1), (8, (1 << 20) + 1)):
            with pytest.raises(ValueError):
                library.without_repeated_frames(max_dist, max_run)
            with pytest.raises(ValueError):
                hvd.pipeline.dedupe_frames_without_repeats_on_device(0, offsets, 64, 64, 1, max_dist, max_run)
    finally:
        library.free()


# ---- 7. DeviceLibrary.without_repeated_frames -------------------------------------------------------------------------------

def _assert_library_equals_host(library, dropped, d_runs, host):
    n = library.n_frames
    lengths = [len(b) // 32 for b in host.hashes]
    assert n == sum(lengths) and library.n_videos == len(lengths)
    assert library.hashes().tobytes() == b"".join(host.hashes)
    assert library.offsets().tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert np.array_equal(library.d_video.to_array(np.int32, n), np.repeat(np.arange(len(lengths)), lengths))
    assert np.array_equal(library.positions(), np.concatenate(host.positions))
    assert np.array_equal(d_runs.to_array(np.int32, n), np.concatenate(host.runs))
    assert dropped.dtype == np.int64 and np.array_equal(dropped, host.dropped)


@pytest.mark.parametrize("max_dist,max_run", [(8, 0), (8, 3), (0, 0), (-1, 0)])
def test_device_library_without_source_positions(gpu, hvd, max_dist, max_run):
    frames, offsets = RH.mixed_library([70, 0, 131, 5, 64, 1, 0], 8, 48)
    frames[200:206] = frames[200]  # (exact repeats, for max_dist 0)
    want_keep, want_run = RH.model_runs(frames, offsets, max_dist, max_run) if max_dist >= 0 else \
        (np.ones(len(frames), bool), np.ones(len(frames), np.int32))
    f2, o2, pos2, want_dropped = RH.model_collapsed(frames, offsets, want_keep)
    host = hvd.without_repeated_frames(RH.blobs(frames, offsets), max_dist, max_run)
    assert host.hashes == RH.blobs(f2, o2) and np.array_equal(host.dropped, want_dropped)
    assert np.array_equal(np.concatenate(host.positions), pos2) and np.array_equal(np.concatenate(host.runs), want_run[want_keep])
    assert all(p.dtype == np.int32 for p in host.positions) and all(r.dtype == np.int32 for r in host.runs)
    assert (want_dropped.sum() > 0) == (max_dist >= 0)
    source = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        before = source.hashes()
        collapsed, dropped, d_runs = source.without_repeated_frames(max_dist, max_run)
        try:
            _assert_library_equals_host(collapsed, dropped, d_runs, host)
            assert collapsed._position_limit == 131
            assert np.array_equal(source.hashes(), before) and source.d_positions is None and source.n_frames == len(frames)
            collapsed.align(collapsed.match_videos())  # the positions are accepted as they are
        finally:
            d_runs.free()
            collapsed.free()
    finally:
        source.free()


def test_device_library_carries_the_positions_of_a_quality_filtered_source(gpu, hvd):
    """The source comes from from_raw_hashes(positions=True) with frames the quality filter dropped, so its positions are not
    its indices; the result's positions are the RAW indices of the frames that survive both filters."""
    raw, raw_offsets = RH.mixed_library([90, 0, 140, 7, 64], 8, 49)
    quality = np.random.default_rng(50).integers(0, 101, len(raw)).astype(np.int32)
    good = quality >= hvd.vpdq.QUALITY_TOLERANCE
    assert not good.all()
    raw_index = np.arange(len(raw)) - np.repeat(raw_offsets[:-1], np.diff(raw_offsets))
    video = np.repeat(np.arange(5), np.diff(raw_offsets))
    kept_offsets = np.concatenate([[0], np.cumsum(np.bincount(video[good], minlength=5))]).astype(np.int64)
    per_video = [raw_index[good][lo:hi] for lo, hi in zip(kept_offsets[:-1], kept_offsets[1:])]
    host = hvd.without_repeated_frames(RH.blobs(raw[good], kept_offsets), 8, positions=per_video)
    assert host.dropped.sum() > 0
    d_h, d_q = gpu.DeviceBuffer.from_array(raw), gpu.DeviceBuffer.from_array(quality)
    try:
        source = hvd.pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, len(raw), raw_offsets, positions=True)
        try:
            assert np.array_equal(source.positions(), raw_index[good])
            collapsed, dropped, d_runs = source.without_repeated_frames(8)
            try:
                _assert_library_equals_host(collapsed, dropped, d_runs, host)
                assert collapsed._position_limit == source._position_limit == 140
                assert np.array_equal(source.positions(), raw_index[good])  # the source is unchanged
            finally:
                d_runs.free()
                collapsed.free()
        finally:
            source.free()
    finally:
        d_h.free()
        d_q.free()
