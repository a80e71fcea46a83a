"""The common-frame filter on the GPU: hvd_dev_vpdq_frame_spread, hvd_dev_common_frames, hvd_dev_gather_kept_i32
and what search.py / pipeline.py build on them, against the model of tests/spread_helpers.py (oracle frame pairs -> spread, a
plain loop -> rule, the oracle's video search on the smaller library). Every comparison is equality on integers."""

import numpy as np
import pytest

import spread_helpers as SH

pytestmark = pytest.mark.gpu


def _T(hvd):
    return hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)


def _device_spread(hvd, frames, offsets, max_dist=None):
    lib_ = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        d = lib_.spread(max_dist)
        try:
            return d.to_array(np.int32, lib_.n_frames)
        finally:
            d.free()
    finally:
        lib_.free()


def _both_spreads(hvd, frames, offsets, max_dist=None):
    host = hvd.search.frame_spread(frames, offsets, max_dist)
    dev = _device_spread(hvd, frames, offsets, max_dist)
    assert host.dtype == np.int32 and np.array_equal(host, dev)
    return host


# ---- 1. distinctness and own video ------------------------------------------------------------------------------------

def test_two_frames_of_one_video_count_once_and_the_own_video_never(gpu, hvd, oracle):
    src = SH.random_hashes(12, 11)
    SH.assert_unrelated(oracle, src)
    x = src[0]
    c = [SH.flipped(x, range(k, k + 7)) for k in (0, 20, 40, 60)]  # four copies of x, 7 flips each
    frames, offsets = SH.library([np.stack([src[1], x, src[2], c[0]]),        # video 0: x and a copy of it
                                  np.stack([c[1], src[3], c[2], src[4]]),     # video 1: two copies
                                  np.stack([src[5], src[6], c[3]])])          # video 2: one copy
    T = _T(hvd)
    got = _both_spreads(hvd, frames, offsets)
    assert np.array_equal(got, SH.model_spread(oracle, frames, offsets, T))
    assert got[1] == 2 and got.tolist() == [0, 2, 0, 2, 2, 0, 2, 0, 0, 0, 2]


# ---- 2. tolerance edge ------------------------------------------------------------------------------------------------

def test_tolerance_edge_and_exact_copies(gpu, hvd, oracle):
    src = SH.random_hashes(6, 12)
    SH.assert_unrelated(oracle, src)
    T = _T(hvd)
    frames, offsets = SH.library([src[0:1], SH.flipped(src[0], range(T))[None], src[1:2], SH.flipped(src[1], range(T + 1))[None],
                                  src[2:3], src[2:3].copy(), src[3:4], SH.flipped(src[3], [200])[None]])
    at_T = _both_spreads(hvd, frames, offsets, T)
    assert at_T.tolist() == [1, 1, 0, 0, 1, 1, 1, 1] and np.array_equal(at_T, SH.model_spread(oracle, frames, offsets, T))
    assert np.array_equal(_both_spreads(hvd, frames, offsets), at_T)  # (the default is T)
    at_0 = _both_spreads(hvd, frames, offsets, 0)
    assert at_0.tolist() == [0, 0, 0, 0, 1, 1, 0, 0] and np.array_equal(at_0, SH.model_spread(oracle, frames, offsets, 0))


# ---- 3. the key table regrows: spread is taken from the last attempt alone -----------------------------------------------

def test_spread_is_not_accumulated_over_table_regrowth(gpu, hvd, oracle):
    V = 300
    src = SH.random_hashes(1 + 2 * V, 13)
    SH.assert_unrelated(oracle, src)
    rng = np.random.default_rng(14)
    videos, shared = [], []
    for v in range(V):
        video = [src[1 + 2 * v], src[2 + 2 * v]]
        video.insert(v % 3, SH.copy_of(src[0], rng))
        shared.append(3 * v + v % 3)
        videos.append(np.stack(video))
    frames, offsets = SH.library(videos)
    want = np.zeros(3 * V, np.int32)
    want[shared] = V - 1  # 300 x 299 = 89 700 keys: more than the first table's 65 536 slots
    assert np.array_equal(SH.model_spread(oracle, frames, offsets, _T(hvd)), want)
    assert np.array_equal(_both_spreads(hvd, frames, offsets), want)


# ---- 4. degenerate libraries ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lengths", [[], [0, 0], [1], [0, 1, 0], [9], [0, 0, 3, 0, 0, 4, 2, 0], [500, 524], [512, 488, 1], [400, 630]],
                         ids=lambda x: "-".join(map(str, x)) or "none")
def test_degenerate_libraries(gpu, hvd, oracle, lengths):
    """No frame, one frame, one video, empty videos at the start, in the middle and at the end of the CSR; 1024 frames (the
    FP4 image's row padding) and counts next to it. Every video holds a copy of one shared source where it has a frame."""
    n = sum(lengths)
    src = SH.random_hashes(n + 1, 15)
    rng = np.random.default_rng(16)
    videos, at = [], 1
    for k in lengths:
        video = src[at:at + k].copy()
        if k:
            video[k // 2] = SH.copy_of(src[0], rng)
        videos.append(video)
        at += k
    frames, offsets = SH.library(videos)
    T = _T(hvd)
    want = SH.model_spread(oracle, frames, offsets, T)
    nonempty = sum(1 for k in lengths if k)
    assert want.sum() == nonempty * (nonempty - 1)
    assert np.array_equal(_both_spreads(hvd, frames, offsets), want)
    # the C entries themselves (the Python layer answers n < 2 without a call)
    lib = gpu.load()
    out = np.full(max(n, 1), -7, np.int32)
    gpu.check(lib.hvd_vpdq_frame_spread(frames.ctypes.data if n else None, offsets.ctypes.data, len(lengths), T, out.ctypes.data))
    assert np.array_equal(out[:n], want)
    # and the whole filter on it
    dropped = SH.model_rule(want, offsets, 0, 100)
    f2, o2, vid2, pos2, per_video = SH.model_filtered(frames, offsets, dropped)
    lib_ = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        filtered, got_dropped = lib_.without_common_frames(0, 100)
        try:
            assert np.array_equal(got_dropped, per_video) and got_dropped.dtype == np.int64
            assert np.array_equal(filtered.hashes(), f2) and np.array_equal(filtered.offsets(), o2)
            assert np.array_equal(filtered.d_video.to_array(np.int32, filtered.n_frames), vid2)
            assert np.array_equal(filtered.positions(), pos2)
        finally:
            filtered.free()
    finally:
        lib_.free()


# ---- 5. the rule on the device against the loop model ---------------------------------------------------------------------

def _device_rule(gpu, spread, offsets, max_videos, max_share):
    n, V = len(spread), len(offsets) - 1
    d_s = gpu.DeviceBuffer.from_array(np.asarray(spread, np.int32)) if n else gpu.DeviceBuffer(4)
    d_o = gpu.DeviceBuffer.from_array(np.asarray(offsets, np.int64))
    d_k = gpu.DeviceBuffer.from_array(np.full(max(n, 1), -7, np.int32))
    try:
        gpu.check(gpu.load().hvd_dev_common_frames(d_s.ptr, d_o.ptr, V, n, max_videos, max_share, d_k.ptr))
        return d_k.to_array(np.int32, n)
    finally:
        for b in (d_s, d_o, d_k):
            b.free()


@pytest.fixture(scope="module")
def rule_case():
    """1 000 videos of 0..300 frames with spreads around M = 3; then the boundary videos (2 of 4, 3 of 4 and 2 of 3 common
    frames; lengths at and next to the bound between the wave and the workgroup path, 2048) and one video of 5 000 frames
    whose common frames include its first and its last."""
    rng = np.random.default_rng(17)
    lengths = rng.integers(0, 301, 1000).tolist() + [4, 4, 3, 2048, 2049, 0, 5000, 7]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    spread = rng.integers(0, 7, int(offsets[-1])).astype(np.int32)
    o = offsets[1000]
    spread[o:o + 11] = [9, 9, 0, 0, 9, 9, 9, 0, 9, 9, 0]
    for v in (1003, 1004, 1006):  # few common frames in the long videos, the ends among them: carriers at 50 %
        lo, hi = offsets[v], offsets[v + 1]
        spread[lo:hi] = rng.integers(0, 4, hi - lo)
        spread[[lo, lo + 1, hi - 2, hi - 1]] = 4
        spread[lo + 70:hi:97] = 6
    return spread, offsets


@pytest.mark.parametrize("max_videos,max_share", [(3, 50), (3, 0), (3, 100), (3, 33), (0, 50), (5, 50), (6, 100)])
def test_device_rule_equals_the_loop_model(gpu, rule_case, max_videos, max_share):
    spread, offsets = rule_case
    want = SH.model_rule(spread, offsets, max_videos, max_share)
    got = _device_rule(gpu, spread, offsets, max_videos, max_share)
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got == 0, want)
    if (max_videos, max_share) == (3, 50):
        o = int(offsets[1000])
        assert (got[o:o + 11] == 0).tolist() == [True, True] + [False] * 9  # 2 of 4 yes; 3 of 4 and 2 of 3 no
        for v in (1003, 1004, 1006):
            assert got[offsets[v]] == 0 and got[offsets[v + 1] - 1] == 0


def test_device_rule_on_one_video_and_on_nothing(gpu):
    spread = np.array([1, 0, 1, 0, 0], np.int32)
    assert _device_rule(gpu, spread, [0, 5], 0, 50).tolist() == [0, 1, 0, 1, 1]
    assert _device_rule(gpu, spread, [0, 5], 0, 39).tolist() == [1, 1, 1, 1, 1]
    assert _device_rule(gpu, spread, [0, 5], 1, 100).tolist() == [1, 1, 1, 1, 1]
    assert _device_rule(gpu, np.zeros(0, np.int32), [0, 0, 0], 0, 50).size == 0


def test_device_rule_takes_its_products_in_64_bits(gpu):
    """43 000 000 common frames in one video: 100 c passes 2^32. All common: dropped at 100 %, kept at 99 %."""
    n = 43_000_000
    d_s, d_o, d_k = gpu.DeviceBuffer(4 * n), gpu.DeviceBuffer.from_array(np.array([0, n], np.int64)), gpu.DeviceBuffer(4 * n)
    try:
        gpu.check(gpu.load().hvd_dev_memset(d_s.ptr, 1, 4 * n))  # every spread 0x01010101
        for max_share, kept in ((100, 0), (99, 1)):
            gpu.check(gpu.load().hvd_dev_common_frames(d_s.ptr, d_o.ptr, 1, n, 5, max_share, d_k.ptr))
            got = d_k.to_array(np.int32, n)
            assert got.min() == kept and got.max() == kept
    finally:
        for b in (d_s, d_o, d_k):
            b.free()


# ---- 6. compaction and positions --------------------------------------------------------------------------------------

def _slate_library(seed):
    """Three slates shared by seven videos. Video 0 has them at its first two positions and at its last one; video 2 is nothing
    but the slates; video 3 is empty; video 1 has one slate in the middle."""
    src = SH.random_hashes(3 + 60, seed)
    rng = np.random.default_rng(seed + 1)
    own = iter(src[3:])
    s = lambda k: SH.copy_of(src[k], rng)  # noqa: E731
    u = lambda: next(own)  # noqa: E731
    videos = [np.stack([s(0), s(1), u(), u(), u(), u(), u(), u(), u(), s(2)]),
              np.stack([u(), s(0), u(), u()]),
              np.stack([s(0), s(1), s(2)]),
              np.zeros((0, 32), np.uint8)]
    videos += [np.stack([u(), u(), s(0), s(1), s(2), u(), u()]) for _ in range(4)]
    return SH.library(videos) + (src,)


def _assert_library_equals(library, want):
    f2, o2, vid2, pos2, _ = want
    assert library.n_frames == len(f2) and library.n_videos == len(o2) - 1
    assert np.array_equal(library.hashes(), f2) and np.array_equal(library.offsets(), o2)
    assert np.array_equal(library.d_video.to_array(np.int32, library.n_frames), vid2)
    assert np.array_equal(library.positions(), pos2)


@pytest.mark.parametrize("max_share", [50, 100])
def test_compaction_without_source_positions(gpu, hvd, oracle, max_share):
    frames, offsets, src = _slate_library(18)
    SH.assert_unrelated(oracle, src)
    spread = SH.model_spread(oracle, frames, offsets, _T(hvd))
    assert spread[0] == 6 and spread[9] == 5
    dropped = SH.model_rule(spread, offsets, 2, max_share)
    want = SH.model_filtered(frames, offsets, dropped)
    assert dropped[[0, 1, 9]].all() and want[4][2] == (3 if max_share == 100 else 0)  # video 2 emptied only at 100 %
    lib_ = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        before = lib_.hashes()
        filtered, got_dropped = lib_.without_common_frames(2, max_share)
        try:
            assert np.array_equal(got_dropped, want[4])
            _assert_library_equals(filtered, want)
            assert filtered._position_limit == 10
            assert np.array_equal(lib_.hashes(), before) and lib_.d_positions is None  # the source is untouched
            # the host path: the same library as bytes and per-video positions
            host = hvd.without_common_frames(SH.blobs(frames, offsets), 2, max_share)
            assert host.hashes == SH.blobs(want[0], want[1]) and np.array_equal(host.dropped, want[4])
            assert np.array_equal(host.spread, spread)
            assert [p.tolist() for p in host.positions] == [want[3][lo:hi].tolist() for lo, hi in zip(want[1][:-1], want[1][1:])]
            # the filtered library aligns on the timeline it had: positions are accepted as they are
            recs = filtered.match_videos()
            assert np.array_equal(recs, oracle.match_videos(want[0], want[1], _T(hvd)))
            filtered.align(recs)
        finally:
            filtered.free()
    finally:
        lib_.free()


def test_compaction_carries_the_positions_of_a_quality_filtered_source(gpu, hvd, oracle):
    """The source comes from from_raw_hashes(positions=True) with frames the quality filter dropped, so its positions are not
    its indices; the result's positions are the RAW indices of the frames that survive both filters."""
    kept_frames, kept_offsets, src = _slate_library(19)
    rng = np.random.default_rng(20)
    junk = iter(SH.random_hashes(200, 21))
    raw, quality, raw_pos, raw_lengths = [], [], [], []
    for lo, hi in zip(kept_offsets[:-1], kept_offsets[1:]):
        at = 0
        for f in range(lo, hi):
            for _ in range(int(rng.integers(0, 3))):  # low-quality frames in front of a kept one
                raw.append(next(junk))
                quality.append(int(rng.integers(0, 31)))
                at += 1
            raw.append(kept_frames[f])
            quality.append(int(rng.integers(31, 101)))
            raw_pos.append(at)
            at += 1
        raw.append(next(junk))  # and one at the end of every video (the empty one included)
        quality.append(0)
        raw_lengths.append(at + 1)
    raw, quality = np.stack(raw), np.array(quality, np.int32)
    raw_offsets = np.concatenate([[0], np.cumsum(raw_lengths)]).astype(np.int64)
    raw_pos = np.array(raw_pos, np.int32)
    assert (raw_pos != np.arange(len(raw_pos)) - np.repeat(kept_offsets[:-1], np.diff(kept_offsets))).any()
    spread = SH.model_spread(oracle, kept_frames, kept_offsets, _T(hvd))
    want = SH.model_filtered(kept_frames, kept_offsets, SH.model_rule(spread, kept_offsets, 2, 50), raw_pos)
    d_h, d_q = gpu.DeviceBuffer.from_array(raw), gpu.DeviceBuffer.from_array(quality)
    try:
        source = hvd.pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, len(raw), raw_offsets, positions=True)
        try:
            assert np.array_equal(source.hashes(), kept_frames) and np.array_equal(source.positions(), raw_pos)
            filtered, got_dropped = source.without_common_frames(2)
            try:
                assert np.array_equal(got_dropped, want[4]) and got_dropped.sum() > 0
                _assert_library_equals(filtered, want)
                assert filtered._position_limit == source._position_limit == max(raw_lengths)
            finally:
                filtered.free()
        finally:
            source.free()
    finally:
        d_h.free()
        d_q.free()
    # the host path carries given positions the same way
    per_video = [raw_pos[lo:hi] for lo, hi in zip(kept_offsets[:-1], kept_offsets[1:])]
    host = hvd.without_common_frames(SH.blobs(kept_frames, kept_offsets), 2, positions=per_video)
    assert np.array_equal(np.concatenate(host.positions), want[3])


def test_gather_kept_i32_past_one_block(gpu):
    rng = np.random.default_rng(22)
    for n in (1, 1023, 1024, 1025, 5000):
        values = rng.integers(-2**31, 2**31, n).astype(np.int32)
        keep = (rng.random(n) < 0.6).astype(np.int32)
        d_in, d_keep, d_out = gpu.DeviceBuffer.from_array(values), gpu.DeviceBuffer.from_array(keep), gpu.DeviceBuffer(4 * n)
        try:
            gpu.check(gpu.load().hvd_dev_gather_kept_i32(d_in.ptr, d_keep.ptr, n, d_out.ptr))
            assert np.array_equal(d_out.to_array(np.int32, int(keep.sum())), values[keep == 1])
        finally:
            for b in (d_in, d_keep, d_out):
                b.free()


# ---- 7. the planted scenario, end to end -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted(hvd, oracle):
    frames, offsets, src = SH.planted_library()
    SH.assert_unrelated(oracle, src)
    return frames, offsets, SH.model_spread(oracle, frames, offsets, _T(hvd))


def test_planted_host_path(gpu, hvd, oracle, planted):
    frames, offsets, spread = planted
    T = _T(hvd)
    intro, want, want_dropped = SH.planted_expectation()
    hashes = SH.blobs(frames, offsets)
    raw = hvd.find_potential_duplicates(hashes, threshold=15)
    assert set(intro) <= set(raw) and len(intro) == 780 and len(raw) == 780 + 66  # the problem: every intro pair is reported
    raw_groups = hvd.find_duplicate_groups(hashes, threshold=15)
    assert len(raw_groups) == 2 and len(raw_groups[0].members) == 40  # ... and chained into one group of 40
    for max_videos in (20, 10):  # at 10 the copies' frames are common too (spread 11): the share rule protects them
        out = hvd.without_common_frames(hashes, max_videos, 50)
        assert np.array_equal(out.spread, spread)
        f2, o2, _, _, per_video = SH.model_filtered(frames, offsets, SH.model_rule(spread, offsets, max_videos, 50))
        assert out.hashes == SH.blobs(f2, o2)
        assert np.array_equal(out.dropped, want_dropped) and np.array_equal(per_video, want_dropped)
        got = hvd.find_potential_duplicates(out.hashes, threshold=15)
        assert got == SH.model_pairs(oracle, f2, o2, T, 15, hvd) == want
        groups = hvd.find_duplicate_groups(out.hashes, threshold=15)
        assert [g.members for g in groups] == [(0, 1), tuple(range(40, 52))]
        hvd.find_excerpts(out.hashes, positions=out.positions)  # the positions are accepted as they are


def test_planted_device_library(gpu, hvd, oracle, planted):
    frames, offsets, spread = planted
    T = _T(hvd)
    _, want, want_dropped = SH.planted_expectation()
    lib_ = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    try:
        for max_videos in (20, 10):
            f2, o2, _, _, _ = SH.model_filtered(frames, offsets, SH.model_rule(spread, offsets, max_videos, 50))
            filtered, dropped = lib_.without_common_frames(max_videos, 50)
            try:
                assert np.array_equal(dropped, want_dropped)
                recs = filtered.match_videos()
                assert np.array_equal(recs, oracle.match_videos(f2, o2, T))
                pairs = hvd.search.similar_video_pairs(recs, filtered.lengths(), 15)
                assert [(int(a), int(b)) for a, b in pairs] == want
            finally:
                filtered.free()
    finally:
        lib_.free()


def test_planted_frames_through_the_chained_pipeline(gpu, hvd, oracle):
    """The same scenario as 64 x 64 gray images (random noise: high PDQ quality, unrelated hashes; a copy is the same image),
    through hash -> quality filter -> spread -> rule -> compaction -> search on one context."""
    plan = SH.planted_plan()
    images = np.random.default_rng(23).integers(0, 256, (SH.planted_sources().shape[0], 64, 64), dtype=np.uint8)
    flat = np.concatenate([images[video] for video in plan])
    raw_offsets = np.concatenate([[0], np.cumsum([len(video) for video in plan])]).astype(np.int64)
    # the model: the product's own hashes and qualities, then the quality filter, the spread, the rule and the oracle's search
    hashes, quality = hvd.vpdq.hash_frames(flat)
    good = quality >= hvd.vpdq.QUALITY_TOLERANCE
    assert good.all()  # (noise has quality 100: the scenario is the planted one)
    frames, offsets = hashes[good], raw_offsets
    T = _T(hvd)
    _, want, want_dropped = SH.planted_expectation()
    spread = SH.model_spread(oracle, frames, offsets, T)
    d_frames = gpu.DeviceBuffer.from_array(flat)
    try:
        for max_videos in (20, 10):
            f2, o2, _, _, _ = SH.model_filtered(frames, offsets, SH.model_rule(spread, offsets, max_videos, 50))
            pairs, recs, dropped, timings = hvd.pipeline.dedupe_frames_without_common_on_device(
                d_frames.ptr, raw_offsets, 64, 64, 1, max_videos, 50, threshold=15)
            assert np.array_equal(recs, oracle.match_videos(f2, o2, T))
            assert [(int(a), int(b)) for a, b in pairs] == SH.model_pairs(oracle, f2, o2, T, 15, hvd) == want
            assert np.array_equal(dropped, want_dropped)
            assert {"hash_ms", "compact_ms", "common_ms", "search_ms"} <= set(timings)
        unfiltered, _, _ = hvd.pipeline.dedupe_frames_on_device(d_frames.ptr, raw_offsets, 64, 64, 1, threshold=15)
        assert len(unfiltered) == 780 + 66
    finally:
        d_frames.free()


# ---- 8. the pair map of the last search survives a spread call ----------------------------------------------------------------

def test_emit_again_after_a_spread_call_returns_the_last_search(gpu, hvd, oracle, planted):
    frames, offsets, _, = hvd.synth.video_hashes(300, seed=24, frames_per_video=(1, 10), copy_fraction=0.4)
    want = oracle.match_videos(frames, offsets, 31)
    assert len(want) > 32
    searched = hvd.pipeline.DeviceLibrary.from_host(frames, offsets)
    other = hvd.pipeline.DeviceLibrary.from_host(planted[0], planted[1])
    try:
        assert np.array_equal(searched.match_videos(31), want)
        d = other.spread()
        assert np.array_equal(d.to_array(np.int32, other.n_frames), planted[2])
        d.free()
        cap = len(want) + 3
        d_out, d_cnt = gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)
        gpu.check(gpu.load().hvd_dev_vpdq_emit_again(d_out.ptr, cap, d_cnt.ptr))
        recs = d_out.to_array(gpu.VMATCH_DTYPE, int(d_cnt.to_array(np.uint64, 1)[0]))
        assert np.array_equal(recs[np.lexsort((recs["b"], recs["a"]))], want)
        d_out.free()
        d_cnt.free()
    finally:
        searched.free()
        other.free()


# ---- 9. bad arguments ---------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_nothing_is_launched(gpu, hvd):
    lib = gpu.load()
    spread, offsets = np.array([5, 5, 0, 0], np.int32), np.array([0, 4], np.int64)
    d_s, d_o = gpu.DeviceBuffer.from_array(spread), gpu.DeviceBuffer.from_array(offsets)
    d_k = gpu.DeviceBuffer.from_array(np.full(4, -7, np.int32))
    try:
        for max_videos, max_share in ((-1, 50), (1, 101), (1, -1)):
            assert lib.hvd_dev_common_frames(d_s.ptr, d_o.ptr, 1, 4, max_videos, max_share, d_k.ptr) == gpu.HVD_ERR_ARG
        assert lib.hvd_dev_vpdq_frame_spread(d_s.ptr, 4, d_s.ptr, 128, d_k.ptr) == gpu.HVD_ERR_ARG
        assert lib.hvd_dev_vpdq_frame_spread(d_s.ptr, 4, d_s.ptr, -1, d_k.ptr) == gpu.HVD_ERR_ARG
        assert lib.hvd_vpdq_frame_spread(None, offsets.ctypes.data, 1, 128, spread.ctypes.data) == gpu.HVD_ERR_ARG
        gpu.check(lib.hvd_dev_sync())
        assert d_k.to_array(np.int32, 4).tolist() == [-7] * 4
        gpu.check(lib.hvd_dev_common_frames(d_s.ptr, d_o.ptr, 1, 4, 1, 50, d_k.ptr))  # (and the good call does write)
        assert d_k.to_array(np.int32, 4).tolist() == [0, 0, 1, 1]
    finally:
        for b in (d_s, d_o, d_k):
            b.free()
    library = hvd.pipeline.DeviceLibrary.from_host(SH.random_hashes(4, 25), offsets)
    try:
        for max_videos, max_share in ((-1, 50), (1, 101)):
            with pytest.raises(ValueError):
                library.without_common_frames(max_videos, max_share)
            with pytest.raises(ValueError):
                hvd.without_common_frames([b"\0" * 64], max_videos, max_share)
            with pytest.raises(ValueError):
                hvd.pipeline.dedupe_frames_without_common_on_device(0, offsets, 64, 64, 1, max_videos, max_share)
    finally:
        library.free()
